// The grouped launch of the bf16 / staged-limb weight-gradient kernels (conv_wgrad_bf16.hip): the jobs of a launch, the host plan that
// says which block computes which (job, dW tile, split), and the block's lookup of it.
//
// The launch is a GROUP: the weight gradients of many layers in one grid (rsis_conv2d_wgrad_batch; see conv_wgrad_tiled.hip), the
// jobs travelling by value in the kernel arguments.  A single weight gradient (rsis_conv2d_wgrad, and every job of the
// deterministic mode) is a group of one job in the PLAIN mode below.
//
// XCD placement of a grouped launch.  A (job, range of consecutive splits) ITEM -- all dW tiles of one job over one range of its
// spatial tiles -- runs on ONE XCD: its blocks re-read the same dy / x pixels once per dW tile (4-16 times each), and only inside
// one L2 are those re-reads hits.  With consecutive block indices spread round-robin over the eight XCDs every XCD fetched the pixels
// again: the bf16 1x1 group read 6.1 GB where 1.5 GB are needed and ran AT the fabric's rate (6 TB/s; rocprofv3 --pmc FETCH_SIZE per
// kernel, tools/step_traffic.py) -- with the MFMA 16x faster than in fp32 these launches are what the memory system lets them be.
// Hardware sends block b to XCD b % 8, so the grid is eight interleaved LANES: lane x is the blocks b = 8 k + x and holds a list of
// items (k ranges); the host balances the lanes by work (longest item first).  (The exact-f32 weight gradients are MFMA-bound: the
// same placement halved their reads and changed their time by nothing, NOTES.md (21).)
// Plain C++ on purpose, as wgrad_block_order.h: tests/test_wgrad_lanes_host.py compiles this header with the host compiler and walks
// every block of every grid through wgb_find.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSIS_LANES_HD __host__ __device__
#else
#define RSIS_LANES_HD
#endif

struct WgradBf16Args {
  const float* dy;   // [B][CoutDy][H][W]
  const float* x;    // [B][Cs][H][W]
  float* dw;         // [Cout][ldo]
  int B, Cs, H, W, Cout;
  int ldo, n_off;
  short interleave_hid;
  short blk;         // dy and x are channel-blocked bf16 tensors (wgrad3_tr_body / wgrad1_tr_body)
  int n_co_tiles, n_n_tiles, n_sp_tiles, tiles_per_split;
};

#define RSIS_WGB_MAXJ 32
#define RSIS_WGB_LANE_ITEMS 28
struct WgradBf16Group {
  int n;
  int lane_n[8];                                  // lane_n[0] < 0: the plain mode, see wgb_find
  int lane_start[8][RSIS_WGB_LANE_ITEMS + 1];     // first k of each item of a lane, ascending; [lane_n] = the lane's block count
  unsigned short lane_split0[8][RSIS_WGB_LANE_ITEMS];   // an item covers the consecutive splits split0, split0 + 1, ... of its job
  unsigned char lane_job[8][RSIS_WGB_LANE_ITEMS];
  WgradBf16Args job[RSIS_WGB_MAXJ];
};
static_assert(sizeof(WgradBf16Group) <= 4000, "kernel arguments are limited to 4 KB");
static_assert(RSIS_WGB_MAXJ <= 256, "lane_job is a byte");

// block -> (job, tile, split); false: a padding block of a short lane.  The block index comes as a callable `bi` (a kernel: one that
// returns blockIdx.x; a host test: any number) and is read inside each branch, unsigned as blockIdx.x is: the divisions of the plain
// mode stay unsigned ones.
// Plain mode (a launch of ONE job on its own): no lanes -- a job with fewer than eight splits, as every job of the deterministic mode,
// would leave XCDs idle behind padding blocks -- but exactly tiles * splits blocks, block b = (tile b % tiles, split b / tiles): the
// order of a (tiles, splits) grid.
template <class BI>
RSIS_LANES_HD inline bool wgb_find(const WgradBf16Group& g, const BI bi, int& job, int& tile, int& split) {
  if (g.lane_n[0] < 0) {                                          // (uniform: a scalar branch)
    const int ntile = g.job[0].n_co_tiles * g.job[0].n_n_tiles;
    const unsigned b = bi();
    job = 0; tile = b % ntile; split = b / ntile;
    return true;
  }
  const unsigned b = bi();
  const int x = b & 7, k = b >> 3;
  const int nl = g.lane_n[x];
  if (k >= g.lane_start[x][nl]) return false;
  int i = 0;
  while (i + 1 < nl && g.lane_start[x][i + 1] <= k) ++i;        // (uniform: scalar code)
  job = g.lane_job[x][i];
  const int kl = k - g.lane_start[x][i], ntile = g.job[job].n_co_tiles * g.job[job].n_n_tiles;
  tile = kl % ntile;
  split = g.lane_split0[x][i] + kl / ntile;
  return true;
}

inline int wgb_cdiv(const long a, const long b) { return (int)((a + b - 1) / b); }

// the dW tiles (bm x bn) and spatial tiles (tw x th) of every job; returns the launch's (dW tile, spatial tile) pairs
inline long wgb_count_tiles(WgradBf16Args* jobs, const int n, const int bm, const int bn, const int tw, const int th) {
  long total = 0;
  for (int j = 0; j < n; ++j) {
    WgradBf16Args& a = jobs[j];
    a.n_co_tiles = wgb_cdiv(a.Cout, bm);
    a.n_n_tiles = wgb_cdiv(a.Cs, bn);
    a.n_sp_tiles = a.B * wgb_cdiv(a.H, th) * wgb_cdiv(a.W, tw);
    total += (long)a.n_co_tiles * a.n_n_tiles * a.n_sp_tiles;
  }
  return total;
}

// the split of a job that is launched on its own (its n_sp_tiles counted)
inline void split_plan(WgradBf16Args& a, const int ntile, const int slots, const bool deterministic) {
  // Every split adds a dW-sized pass of fp32 atomics, and those run at ~0.3 T atomics/s whatever the layer: measured on the
  // trunk shapes at batch 32 (tools/exp/bf16_shape_sweep.py), one block per CU (256 slots) beats two (512) on every layer --
  // 4.4 vs 5.7 ms per step -- although the main loop alone is no faster (2.7 vs 2.6 ms): the second block only buys atomics.
  int nsplit = ntile >= slots ? 1 : slots / ntile;
  if (nsplit > 256) nsplit = 256;
  if (nsplit > a.n_sp_tiles / 2) nsplit = a.n_sp_tiles / 2;
  if (nsplit < 1 || deterministic) nsplit = 1;
  a.tiles_per_split = wgb_cdiv(a.n_sp_tiles, nsplit);
}

struct WgbPlan { int blocks, jobs; };      // grid size of the launch; jobs of the list it holds

// ONE job on its own: split_plan, plain mode
inline WgbPlan wgb_plan_alone(WgradBf16Group& g, WgradBf16Args& a, const bool deterministic) {
  const int ntile = a.n_co_tiles * a.n_n_tiles;
  split_plan(a, ntile, 256, deterministic);
  g = WgradBf16Group{};
  g.n = 1;
  g.lane_n[0] = -1;
  g.job[0] = a;
  return WgbPlan{ntile * wgb_cdiv(a.n_sp_tiles, a.tiles_per_split), 1};
}

// The next launch of a list of jobs (tiles counted; `total` = wgb_count_tiles of the WHOLE list, so that every launch of it cuts
// its jobs alike): every block walks ~total / target_blocks spatial tiles -- in deterministic mode all of its job's -- and the
// blocks are placed on the XCD lanes.  Holds as many of the first n jobs as RSIS_WGB_MAXJ and the 8 * RSIS_WGB_LANE_ITEMS items allow.
inline WgbPlan wgb_plan_lanes(WgradBf16Group& g, const WgradBf16Args* jobs, const int n, const long total, const long target_blocks,
                              const bool deterministic) {
  long L = (total + target_blocks - 1) / target_blocks;
  if (L < 2) L = 2;
  if (deterministic) L = 1L << 40;
  g = WgradBf16Group{};
  // items of this launch: a job with up to 8 splits is one item per split, a job with more is 8 items of consecutive splits
  struct Item { int job, split, blocks; long work; };
  Item items[8 * RSIS_WGB_LANE_ITEMS];
  int ni = 0, nj = 0;
  while (nj < n && nj < RSIS_WGB_MAXJ) {
    WgradBf16Args a = jobs[nj];
    int nsplit = wgb_cdiv(a.n_sp_tiles, L);
    if (nsplit < 1) nsplit = 1;
    if (nsplit > 60000) nsplit = 60000;                         // (lane_split0 is 16 bits)
    a.tiles_per_split = wgb_cdiv(a.n_sp_tiles, nsplit);
    nsplit = wgb_cdiv(a.n_sp_tiles, a.tiles_per_split);
    const int nit = nsplit < 8 ? nsplit : 8;
    if (ni + nit > 8 * RSIS_WGB_LANE_ITEMS) break;              // (nj >= 1 here: one job is at most 8 items)
    const int ntile = a.n_co_tiles * a.n_n_tiles;
    for (int it = 0; it < nit; ++it) {
      const int s0 = (int)((long)nsplit * it / nit), s1 = (int)((long)nsplit * (it + 1) / nit);
      const long tiles = (long)(s1 < nsplit ? (long)s1 * a.tiles_per_split : a.n_sp_tiles) - (long)s0 * a.tiles_per_split;
      items[ni++] = Item{nj, s0, ntile * (s1 - s0), (long)ntile * tiles};
    }
    g.job[nj++] = a;
  }
  g.n = nj;
  for (int x = 1; x < ni; ++x)           // longest item first onto the least loaded lane that still has a free slot
    for (int y = x; y > 0 && items[y].work > items[y - 1].work; --y) { const Item t = items[y]; items[y] = items[y - 1]; items[y - 1] = t; }
  long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int blocks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < ni; ++i) {
    int best = -1;
    for (int x = 0; x < 8; ++x)
      if (g.lane_n[x] < RSIS_WGB_LANE_ITEMS && (best < 0 || load[x] < load[best])) best = x;
    const int e = g.lane_n[best]++;
    g.lane_start[best][e] = blocks[best];
    g.lane_job[best][e] = (unsigned char)items[i].job;
    g.lane_split0[best][e] = (unsigned short)items[i].split;
    blocks[best] += items[i].blocks;
    load[best] += items[i].work;
  }
  int maxb = 0;
  for (int x = 0; x < 8; ++x) { g.lane_start[x][g.lane_n[x]] = blocks[x]; if (blocks[x] > maxb) maxb = blocks[x]; }
  return WgbPlan{8 * maxb, nj};
}
