// CVPPP leaf segmentation challenge measures on the device (gfx950): SymmetricBestDice, FgBgDice, DiffFGLabels of N pairs of 8-bit label
// images (result `in`, ground truth `gt`) of different sizes, in two grouped launches (definitions: include/rsis_hip.h and
// rsis_amd/cvppp_eval.py; the challenge scored them with Matlab scripts, reference src/CVPPP/).  Everything is an integer count or a
// float64 expression of such counts evaluated in a fixed order, so nothing depends on the schedule.
//   label_contingency_kernel : the joint counts o_ij = #{in == i and gt == j} of every pair.  The images lie in one byte pool; a pair is
//     cut into blocks of LC_CHUNK pixels, a thread reads 16 pixels of each image with one 16-byte load.  The table of a leaf image is
//     60-80 % one (background, background) cell, and same-address atomics serialise (NOTES.md (6c) / (8b)), so counts are merged before
//     they leave the CU, in three stages:
//       1. a lane keeps ONE open run (key = in << 8 | gt, count) across all the pixels it reads; a 16-pixel cell whose 32 bytes are one
//          key costs 8 compares, an all-background lane issues a single atomic in the whole kernel;
//       2. a closed run adds into a block-private LC_WIN x LC_WIN window (labels 0 .. 63 of both images, 16 KiB of LDS: every CVPPP image
//          and every label image the decoder can write, T <= 64); a key outside the window adds directly to the global table, one atomic
//          per RUN (the full 256 x 256 table would be 256 KiB and does not fit the 160 KiB of a CU);
//       3. the block adds the non-zero cells of its window to the global table: at most one global atomic per cell and block.
//     Global table: dense, counts[table_off + i * 256 + j], uint32, 256 KiB per pair, zeroed by the call (no min / max pre-pass: it would
//     read every image twice).  Pairs need not start on 16-byte boundaries: the pixels before the first 16-byte boundary of `in` and the
//     last npix % 16 go one per thread; when `gt` sits at another offset modulo 16 its 16 bytes are cut out of the two aligned cells
//     they span.
//   label_scores_kernel      : one block per pair, table (one pass) -> marginals -> lo / hi of both images -> BestDice both ways (maxima are exact in
//     any order; the two sums run sequentially in ascending label order in ONE thread) -> six float64 scores.
#include "common.h"
#include "launchers.h"

typedef unsigned long long u64;

#define LC_T 256
#define LC_ITERS 8
#define LC_UNROLL 4
#define LC_CELLS (LC_T * LC_ITERS)          // 16-pixel cells per block
#define LC_CHUNK (LC_CELLS * 16)            // pixels per block
#define LC_WIN 64
#define LC_TABLE 65536                      // 256 x 256 counts per pair

__device__ __forceinline__ void lc_flush(unsigned key, unsigned cnt, unsigned* win, unsigned* tab) {
  if (!cnt) return;
  const unsigned i = key >> 8, j = key & 255u;
  if (i < LC_WIN && j < LC_WIN) atomicAdd(&win[i * LC_WIN + j], cnt);
  else atomicAdd(tab + key, cnt);                                 // (key == i * 256 + j)
}

__device__ __forceinline__ void lc_push(unsigned key, unsigned n, unsigned& cur, unsigned& cnt, unsigned* win, unsigned* tab) {
  if (key == cur) {
    cnt += n;
  } else {
    lc_flush(cur, cnt, win, tab);
    cur = key;
    cnt = n;
  }
}

// 16 pixels: a = bytes of `in`, g = bytes of `gt`
__device__ __forceinline__ void lc_cell(const uint4 a, const uint4 g, unsigned& cur, unsigned& cnt, unsigned* win, unsigned* tab) {
  const unsigned ab = a.x & 255u, gb = g.x & 255u;
  const bool uni = (a.x == ab * 0x01010101u) & (a.y == a.x) & (a.z == a.x) & (a.w == a.x) & (g.x == gb * 0x01010101u) & (g.y == g.x) &
                   (g.z == g.x) & (g.w == g.x);
  if (uni) {
    lc_push((ab << 8) | gb, 16u, cur, cnt, win, tab);
    return;
  }
  const unsigned av[4] = {a.x, a.y, a.z, a.w}, gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) lc_push((((av[q] >> (8 * k)) & 255u) << 8) | ((gv[q] >> (8 * k)) & 255u), 1u, cur, cnt, win, tab);
}

// the 16 bytes at pool + G (G % 16 == s != 0) out of the two aligned cells they span
__device__ __forceinline__ uint4 lc_load_shifted(const unsigned char* __restrict__ pool, long G, int s) {
  const uint4* p = reinterpret_cast<const uint4*>(pool + (G - s));
  const uint4 A = p[0], B = p[1];
  const unsigned w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
  const int q = s >> 2, b8 = (s & 3) * 8;
  unsigned t[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) t[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
  uint4 r;
  r.x = (unsigned)(((((u64)t[1]) << 32) | t[0]) >> b8);
  r.y = (unsigned)(((((u64)t[2]) << 32) | t[1]) >> b8);
  r.z = (unsigned)(((((u64)t[3]) << 32) | t[2]) >> b8);
  r.w = (unsigned)(((((u64)t[4]) << 32) | t[3]) >> b8);
  return r;
}

// jobs[j] = {in_off, gt_off, npix, table_off, block_begin, 0, 0, 0}; pool is 16-byte aligned, table_off a multiple of 4
__global__ __launch_bounds__(LC_T) void label_contingency_kernel(const unsigned char* __restrict__ pool, long pool_len,
                                                                 const long long* __restrict__ jobs, int njobs, unsigned int* __restrict__ counts,
                                                                 long counts_len) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {                                               // last job whose block_begin <= b
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[8 * (long)mid + 4] <= b) lo = mid; else hi = mid - 1;
  }
  const long long* J = jobs + 8 * (long)lo;
  const long in_off = J[0], gt_off = J[1], npix = J[2], table_off = J[3];
  const long tb = b - J[4];
  if (in_off < 0 || gt_off < 0 || npix < 1 || npix >= (1L << 32) || in_off > pool_len - npix || gt_off > pool_len - npix || table_off < 0 ||
      (table_off & 3) || table_off > counts_len - LC_TABLE || tb < 0 || tb >= (npix + LC_CHUNK - 1) / LC_CHUNK)
    return;                                                       // (block-uniform) a job that does not fit the buffers touches nothing
  unsigned int* tab = counts + table_off;
  const unsigned char* pin = pool + in_off;
  const unsigned char* pgt = pool + gt_off;
  __shared__ unsigned int win[LC_WIN * LC_WIN];
  for (int c = tid; c < LC_WIN * LC_WIN; c += LC_T) win[c] = 0;
  __syncthreads();
  long head = (16 - (in_off & 15)) & 15;                          // pixels before the first 16-byte boundary of `in`
  if (head > npix) head = npix;
  const long ncells = (npix - head) >> 4;
  const int s = (int)((gt_off + head) & 15);                      // where `gt` stands when `in` is aligned
  unsigned cur = 0, cnt = 0;
  const long c0 = tb * LC_CELLS, c1 = c0 + LC_CELLS < ncells ? c0 + LC_CELLS : ncells;
  if (s == 0) {
    for (int it = 0; it < LC_ITERS; it += LC_UNROLL) {
      uint4 a[LC_UNROLL], g[LC_UNROLL];
#pragma unroll
      for (int u = 0; u < LC_UNROLL; ++u) {
        const long c = c0 + (long)(it + u) * LC_T + tid;
        if (c < c1) {
          a[u] = *reinterpret_cast<const uint4*>(pin + head + 16 * c);
          g[u] = *reinterpret_cast<const uint4*>(pgt + head + 16 * c);
        }
      }
#pragma unroll
      for (int u = 0; u < LC_UNROLL; ++u)
        if (c0 + (long)(it + u) * LC_T + tid < c1) lc_cell(a[u], g[u], cur, cnt, win, tab);
    }
  } else {
    for (int it = 0; it < LC_ITERS; ++it) {
      const long c = c0 + (long)it * LC_T + tid;
      if (c >= c1) continue;
      const long p = head + 16 * c, G = gt_off + p;
      if (G - s + 32 <= pool_len) {
        lc_cell(*reinterpret_cast<const uint4*>(pin + p), lc_load_shifted(pool, G, s), cur, cnt, win, tab);
      } else {                                                    // the second aligned cell would end past the pool: byte loads
        for (int k = 0; k < 16; ++k) lc_push(((unsigned)pin[p + k] << 8) | pgt[p + k], 1u, cur, cnt, win, tab);
      }
    }
  }
  if (tb == 0) {                                                  // the pixels outside the 16-byte cells: fewer than 16 at either end
    const long t0 = head + 16 * ncells;
    if (tid < head) lc_push(((unsigned)pin[tid] << 8) | pgt[tid], 1u, cur, cnt, win, tab);
    if (t0 + tid < npix) lc_push(((unsigned)pin[t0 + tid] << 8) | pgt[t0 + tid], 1u, cur, cnt, win, tab);
  }
  lc_flush(cur, cnt, win, tab);
  __syncthreads();
  for (int c = tid; c < LC_WIN * LC_WIN; c += LC_T) {
    const unsigned v = win[c];
    if (v) atomicAdd(tab + (c / LC_WIN) * 256 + (c % LC_WIN), v);
  }
}

// 2 o / (n + m): one float64 division of two integers; 0 / 0 never wins a maximum and counts as 0
__device__ __forceinline__ double ls_dice(unsigned o, unsigned n, unsigned m) {
  const u64 den = (u64)n + (u64)m;
  return den ? (double)(2 * (u64)o) / (double)den : 0.0;
}

#define LS_T 256
// scores[pair] = {SymmetricBestDice, FgBgDice, AbsDiffFGLabels, DiffFGLabels, BestDice(in, gt), BestDice(gt, in)}
__global__ __launch_bounds__(LS_T) void label_scores_kernel(const unsigned int* __restrict__ counts, long counts_len, const long long* __restrict__ jobs,
                                                            double* __restrict__ scores) {
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long table_off = jobs[8 * (long)pair + 3];
  if (table_off < 0 || (table_off & 3) || table_off > counts_len - LC_TABLE) return;   // (block-uniform; rows are read as 16-byte cells)
  const unsigned int* T = counts + table_off;
  __shared__ unsigned int n[256], m[256], total;
  __shared__ int rng[4];                                           // lo_in, hi_in, lo_gt, hi_gt
  __shared__ double bi[256], bg[256];
  if (tid == 0) { total = 0; rng[0] = 256; rng[1] = -1; rng[2] = 256; rng[3] = -1; }
  m[tid] = 0;
  __syncthreads();
  unsigned c4[4] = {0, 0, 0, 0};                                   // one pass over the table: a wave per row, a lane per 4 columns
  for (int r = 0; r < 64; ++r) {
    const int row = wv * 64 + r;
    const uint4 v = *reinterpret_cast<const uint4*>(T + row * 256 + lane * 4);
    c4[0] += v.x; c4[1] += v.y; c4[2] += v.z; c4[3] += v.w;
    unsigned rs = v.x + v.y + v.z + v.w;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rs += __shfl_down(rs, o, 64);
    if (lane == 0) n[row] = rs;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c4[k]) atomicAdd(&m[lane * 4 + k], c4[k]);                 // the four waves' column sums (integers: any order)
  __syncthreads();
  if (n[tid]) { atomicMin(&rng[0], tid); atomicMax(&rng[1], tid); atomicAdd(&total, n[tid]); }
  if (m[tid]) { atomicMin(&rng[2], tid); atomicMax(&rng[3], tid); }
  __syncthreads();
  if (total == 0) return;                                          // (block-uniform) nothing was counted: the scores stay zero
  const int li = rng[0], hi_ = rng[1], lg = rng[2], hg = rng[3];
  for (int i = li + wv; i <= hi_; i += LS_T / 64) {                 // BestDice(in, gt): row i against every column of the range
    double best = 0.0;
    for (int j = lg + lane; j <= hg; j += 64) {
      const double d = ls_dice(T[i * 256 + j], n[i], m[j]);
      best = d > best ? d : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double t = __shfl_down(best, o, 64);
      best = t > best ? t : best;
    }
    if (lane == 0) bi[i] = best;
  }
  if (lg + tid <= hg) {                                             // BestDice(gt, in): column j against every row of the range
    const int j = lg + tid;
    double best = 0.0;
    for (int i = li; i <= hi_; ++i) {
      const double d = ls_dice(T[i * 256 + j], m[j], n[i]);
      best = d > best ? d : best;
    }
    bg[j] = best;
  }
  __syncthreads();
  if (tid == 0) {
    double si = 0.0, sg = 0.0;
    for (int i = li; i <= hi_; ++i) si += bi[i];                    // ascending, sequential: the stated order
    for (int j = lg; j <= hg; ++j) sg += bg[j];
    const double bdi = si / (double)(hi_ - li + 1), bdg = sg / (double)(hg - lg + 1);
    const u64 fin = (u64)total - n[li], fgt = (u64)total - m[lg];
    const u64 both = (u64)total - n[li] - m[lg] + T[li * 256 + lg];  // |F_in and F_gt| by inclusion / exclusion
    const double zero = 0.0;
    const double fgbg = (fin + fgt) ? (double)(2 * both) / (double)(fin + fgt) : zero / zero;
    const int diff = (hi_ - li) - (hg - lg);
    double* S = scores + 6 * (long)pair;
    S[0] = bdi < bdg ? bdi : bdg;
    S[1] = fgbg;
    S[2] = (double)(diff < 0 ? -diff : diff);
    S[3] = (double)diff;
    S[4] = bdi;
    S[5] = bdg;
  }
}

long rsis_l_label_contingency_blocks(long npix) { return (npix + LC_CHUNK - 1) / LC_CHUNK; }

int rsis_l_label_contingency_batch(const unsigned char* pool, long pool_len, const long long* jobs, int njobs, int total_blocks,
                                   unsigned int* counts, long counts_len, hipStream_t st) {
  if (rsis_zero_async(counts, sizeof(unsigned int) * (size_t)counts_len, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(label_contingency_kernel, dim3(total_blocks), dim3(LC_T), 0, st, pool, pool_len, jobs, njobs, counts, counts_len);
  return rsis_check_launch();
}

int rsis_l_label_scores_batch(const unsigned int* counts, long counts_len, const long long* jobs, int njobs, double* scores, hipStream_t st) {
  if (rsis_zero_async(scores, sizeof(double) * 6 * (size_t)njobs, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(label_scores_kernel, dim3(njobs), dim3(LS_T), 0, st, counts, counts_len, jobs, scores);
  return rsis_check_launch();
}
