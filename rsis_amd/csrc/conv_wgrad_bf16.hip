// Weight gradient of the stride-1 "same" convolutions (3x3/p1 and 1x1/p0) with bf16 operands / fp32 accumulation on
// v_mfma_f32_32x32x16_bf16 (the `-dtype bf16` path):
//     dW[co][ci][r][s] += sum_{b,y,x} dy[b][co][y][x] * x[b][ci][y+r-pad][x+s-pad]
// (autograd of nn.Conv2d in reference src/modules/clstm.py:17,44 -- the ConvLSTM gates, time-batched over T*B images --
//  model.py:43-47 and the 1x1 / 3x3 convs of the torchvision bottlenecks).  dy, x and dW are fp32 (NCHW / reference layout);
//  the operands are rounded to bf16 while they are staged into LDS (IN = 1 / 0: rows of whole / ragged float4s).  Channel-blocked bf16
//  operands (conv_blk.hip: cells of 8 channels x 1 pixel) take the DMA / transposing-read kernels further down (wgrad3_tr_body,
//  wgrad1_tr_body): no staging pass at all.
//
// The PIXELS are the reduction axis, and NCHW has them contiguous: a lane's 8 K values are 8 consecutive pixels of one row,
// i.e. one 16-byte LDS cell, for dy (A operand, rows = co) and for x (B operand) alike.
//   * 1x1: a plain GEMM D[co][ci] over BM x BN tiles, both operand tiles staged as [row][64 px] (+16 B row padding: the 32 rows
//     a wave reads land on distinct banks).
//   * 3x3: the lanes of the B operand are 32 INPUT CHANNELS and the 9 taps are 9 accumulator tiles of the wave, so the tap
//     (and with it the 1-pixel shift of the window) is a compile-time constant: per patch row the wave reads the aligned 16-byte
//     window plus one dword on either side and builds the s = 0 / s = 2 windows with 4 v_alignbit_b32 each -- 3 LDS reads and
//     8 VALU per 3 MFMAs.  The input patch (with halo) is staged once per tile, not 9 times.  The 32 x 288 accumulator slab of
//     a wave is transposed through LDS before the fp32 atomics so that consecutive lanes hit consecutive dW addresses.
// Ragged maps (the 7/14/28/56/112-pixel pyramid of 224 x 224 inputs) need no special case: out-of-map pixels are zero-filled
// when the tile is staged.  Split-K over spatial tiles / images with fp32 atomics into dW, as conv_wgrad_tiled.hip.
// One launch path: every weight gradient, a single one included, runs on the *_group_kernel of its body through wgb_launch_bucket, and
// wgb_key alone says which instantiation a layer gets.
//
// LIMBS = 1 of the two register-staged bodies (wgrad3_limb_group_kernel / wgrad1_limb_group_kernel) is an fp32 path: the operands
// are not rounded but split into three exact bf16 limbs (limb_split.h) ONCE per staged element, while its cell is stored -- three
// limb planes per stage -- and the MFMA loop runs the six limb products of the LIMB loop of conv_wgrad_tiled.hip on ready fragments,
// with no split arithmetic in it (that loop splits every value after every ds_read: up to 18 times per element of a 3x3).  Which
// fp32 jobs take it is a measured table over job classes (wgl_class / wgl_class_mask; today the 3x3 jobs on 32-wide tiles whose
// source is a multiple of 32 channels), in deterministic mode none.  RSIS_WGRAD_LIMBS: unset = the tables; 0 / all = every job on the
// f32 loop / the register-split loop of conv_wgrad_tiled.hip; reg = the tables with no staged class (A/B inside one build);
// staged = every fp32 job rsis_wgrad_bf16_supported accepts runs here, and one it does not is RSIS_ERR_UNSUPPORTED.
#include "common.h"
#include "launchers.h"
#include "limb_split.h"
#include "wgrad_lanes.h"
#include "wgrad_parts.h"
#include <stdlib.h>
#include <string.h>

// ------------------------------------------------------------------------------------------------
// 3x3: block = BM dy rows x 32 input channels x 9 taps; wave = 32 rows x 32 channels x 9 taps, the 4 / (BM / 32) wave copies of a
// row group take alternate 16-pixel reduction steps.
// ------------------------------------------------------------------------------------------------
// LIMBS = 1 (fp32 weight gradients on three exact bf16 limbs per operand, six products per K16 step, as the LIMB loop of
// conv_wgrad_tiled.hip -- but every staged element is split ONCE, while its cell is stored): the stage is three PLANES of the bf16
// stage's layout, plane l = limb l of every element, and the MFMA loop reads ready limb fragments: per K16 step 3 dy reads, and
// per patch row and plane the 3 reads + 8 v_alignbit_b32 of the bf16 loop, for 6 x 9 MFMAs.  The limb pair is the outer loop and
// the tap the inner one: consecutive MFMAs never share an accumulator.  Three planes leave no room for the second buffer: ONE
// stage, the next tile prefetched into registers under the MFMAs and split + stored between two barriers.
template <int BM, int TW, int IN, int LIMBS = 0>
__device__ __forceinline__ void wgrad3_bf16_body(const WgradBf16Args& p, const int bx, const int by) {
#if __HIP_DEVICE_COMPILE__
  using Geo = W3Stage<BM, TW, LIMBS>;
  constexpr int TH = Geo::TH, GPR = Geo::GPR, NG = Geo::NG, KSTEPS = Geo::KSTEPS;
  constexpr int PH = Geo::PH, XG = Geo::XG, PWP = Geo::PWP, ARS = Geo::ARS, CHSB = Geo::CHSB;
  constexpr int A_BYTES = Geo::A_BYTES, ST_BYTES = Geo::ST_BYTES, NTA = Geo::NTA, XT = Geo::XT, NTX = Geo::NTX;
  constexpr int NPL = Geo::NPL, NPROD = LIMBS ? RSIS_LIMB_PRODUCTS : 1;
  constexpr bool FLUSH = LIMBS && BM == 128;                      // (the chain of MFMA accumulations is cut per tile, see `tot`)
  constexpr int WGM = BM / 32, KSPW = 4 / WGM, NGG = KSTEPS / KSPW;
  static_assert(WGM * KSPW == 4 && KSTEPS % KSPW == 0, "config");
  char* const lds = wgb_stage_lds<Geo::LDS_BYTES, LIMBS != 0>();

  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WGM, wk = wave / WGM;
  const int H = p.H, W = p.W, HW = H * W, Cs = p.Cs, Cout = p.Cout;
  const int co_t = bx % p.n_co_tiles, n_t = bx / p.n_co_tiles;
  const int co0 = co_t * BM, ci0 = n_t * 32;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int t_begin = by * p.tiles_per_split;
  const int t_end = min(t_begin + p.tiles_per_split, p.n_sp_tiles);
  if (t_begin >= t_end) return;

  // ---- loop-invariant parts of the staging tasks ----
  // (LIMBS at two blocks per CU: 20 registers the MFMA loop has no room for.  Kept, they were spilled, and a reload between the
  //  prefetch loads waits for every load before it: the tile's loads went out one round trip after the other.  There they are
  //  computed again per tile, before the loads and before the stores, from a thread index the compiler cannot see through.)
  int a_off[NTA], a_y[NTA], a_x[NTA], a_lds[NTA];
  int x_off[NTX], x_y[NTX], x_x[NTX], x_lds[NTX];
#define W3_TASKS(T)                                                                                                \
  {                                                                                                                \
    _Pragma("unroll") for (int i = 0; i < NTA; ++i) {                                                              \
      const int e = (T) + i * 256;                                                                                 \
      const int row = e / NG, G = e % NG;                                                                          \
      a_y[i] = G / GPR; a_x[i] = (G % GPR) * 8;                                                                    \
      a_off[i] = co0 + row < Cout ? row * HW + a_y[i] * W + a_x[i] : -1;                                           \
      a_lds[i] = row * ARS + G * 16;                                                                               \
    }                                                                                                              \
    _Pragma("unroll") for (int i = 0; i < NTX; ++i) {                                                              \
      const int e = (T) + i * 256;                                                                                 \
      const int cl = e / (PH * XG), rem = e - cl * (PH * XG);                                                      \
      const int py = rem / XG, xg = rem - py * XG;                                                                 \
      x_y[i] = py - 1; x_x[i] = (xg - 1) * 8;                                                                      \
      x_off[i] = (e < XT && ci0 + cl < Cs) ? cl * HW + x_y[i] * W + x_x[i] : (int)0x40000000;   /* (flag: never valid) */ \
      x_lds[i] = cl * CHSB + (py * PWP + xg * 8) * 2;                                                              \
    }                                                                                                              \
  }
  constexpr bool RETASK = LIMBS && BM < 128;
#define W3_RETASK() if constexpr (RETASK) { int tv = tid; asm volatile("" : "+v"(tv)); W3_TASKS(tv) }
  W3_TASKS(tid)

  // ---- per-lane LDS read bases (bytes) ----
  const int a_base = (wm * 32 + l31) * ARS + hi * 16;
  // step g covers groups 2g (lanes 0-31) and 2g+1 (lanes 32-63): pixel (y, x8*8) of the tile, patch column 8 + x8*8
  int bo[NGG];
#pragma unroll
  for (int gg = 0; gg < NGG; ++gg) {
    const int G = 2 * (gg * KSPW + wk) + hi;
    bo[gg] = l31 * CHSB + ((G / GPR) * PWP + (G % GPR) * 8 + 8) * 2;
  }

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // The bf16 MFMA does not round its sum into the accumulator to nearest as the f32 MFMA's fmaf chain does: over a chain of six
  // MFMAs per K16 step the error grows with the chain's LENGTH, not its square root (measured: a wave that walked 12 K16 steps of a
  // 1x1 was 4.6 x as far from float64 as one that walked 4; the f32 loop 1.4 x).  So a wave that walks every K16 step of a tile
  // itself (BM = 128, and every 1x1 tile) starts each tile from zero accumulators and adds them to `tot` on the VALU, round to
  // nearest: at most 24 MFMAs per chain.  BM = 64 / 32 deal the K16 steps over 2 / 4 wave copies -- chains half / a quarter as
  // long per tile -- and at two blocks per CU have no registers for a second set of nine tiles.
  [[maybe_unused]] f32x16 tot[FLUSH ? 9 : 1];
  if constexpr (FLUSH) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) tot[t][r] = 0.f;
  }

  WgCursor cs(t_begin, tiles_x, tiles_y);                          // (scalar; of the NEXT tile to load)

  Task8<IN == 1> ra[NTA], rxp[NTX];
#define W3_LOAD()                                                                                                  \
  {                                                                                                                \
    const int y0 = cs.ty * TH, x0 = cs.tx * TW;                                                                          \
    const float* ab = p.dy + ((size_t)cs.tb * Cout + co0) * HW;                                                       \
    const __amdgpu_buffer_rsrc_t ra_ = __builtin_amdgcn_make_buffer_rsrc((void*)ab, 0, (Cout - co0) * HW * 4, 0x00020000); \
    const int tsc = y0 * W + x0;                                                                                   \
    _Pragma("unroll") for (int i = 0; i < NTA; ++i)                                                                \
      ra[i].load(ra_, a_off[i] + tsc, a_off[i] >= 0 && y0 + a_y[i] < H, x0 + a_x[i], W);                           \
    const float* xb = p.x + ((size_t)cs.tb * Cs + ci0) * HW;                                                          \
    const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, (Cs - ci0) * HW * 4, 0x00020000); \
    _Pragma("unroll") for (int i = 0; i < NTX; ++i)                                                                \
      rxp[i].load(rx_, x_off[i] + tsc, x_off[i] < 0x20000000 && (unsigned)(y0 + x_y[i]) < (unsigned)H, x0 + x_x[i], W); \
    cs.next(tiles_x, tiles_y);                                                                                     \
  }
#define W3_STORE(BUF)                                                                                              \
  {                                                                                                                \
    char* st = lds + (BUF) * ST_BYTES;                                                                             \
    if constexpr (LIMBS) {                                                                                         \
      u32x4 c[3];                                                                                                  \
      _Pragma("unroll") for (int i = 0; i < NTA; ++i) {                                                            \
        ra[i].limb_cells(c);                                                                                       \
        _Pragma("unroll") for (int l = 0; l < 3; ++l) *(u32x4*)(st + l * ST_BYTES + a_lds[i]) = c[l];              \
      }                                                                                                            \
      _Pragma("unroll") for (int i = 0; i < NTX; ++i)                                                              \
        if (XT % 256 == 0 || tid + i * 256 < XT) {                                                                 \
          rxp[i].limb_cells(c);                                                                                    \
          _Pragma("unroll") for (int l = 0; l < 3; ++l) *(u32x4*)(st + l * ST_BYTES + A_BYTES + x_lds[i]) = c[l];  \
        }                                                                                                          \
    } else {                                                                                                       \
      _Pragma("unroll") for (int i = 0; i < NTA; ++i) *(u32x4*)(st + a_lds[i]) = ra[i].cell();                     \
      _Pragma("unroll") for (int i = 0; i < NTX; ++i)                                                              \
        if (XT % 256 == 0 || tid + i * 256 < XT) *(u32x4*)(st + A_BYTES + x_lds[i]) = rxp[i].cell();               \
    }                                                                                                              \
  }

  W3_LOAD() W3_STORE(0)
  __syncthreads();
  const int ntl = t_end - t_begin;
  for (int t = 0; t < ntl; ++t) {
    const int cur = LIMBS ? 0 : t & 1;
    if (t + 1 < ntl) { W3_RETASK() W3_LOAD() }
    const char* As = lds + cur * ST_BYTES + a_base;
    const char* Xs = lds + cur * ST_BYTES + A_BYTES;
#pragma unroll
    for (int gg = 0; gg < NGG; ++gg) {
      bf16x8 a[NPL];
#pragma unroll
      for (int l = 0; l < NPL; ++l) a[l] = __builtin_bit_cast(bf16x8, *(const u32x4*)(As + l * ST_BYTES + (gg * KSPW + wk) * 32));
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        bf16x8 w[NPL][3];                                           // [plane][tap s]
#pragma unroll
        for (int l = 0; l < NPL; ++l) wg3_windows(Xs + l * ST_BYTES + bo[gg] + r * PWP * 2, w[l]);
#pragma unroll
        for (int q = 0; q < NPROD; ++q)
#pragma unroll
          for (int s = 0; s < 3; ++s)
            acc[r * 3 + s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[LIMBS ? RSIS_LIMB_PA(q) : 0], w[LIMBS ? RSIS_LIMB_PB(q) : 0][s], acc[r * 3 + s], 0, 0, 0);
        // (LIMBS on 32-wide tiles at two blocks per CU: the windows of the next row are not built above this row's MFMAs -- two
        //  rows of them live at once spilled 21 registers, some of them reloaded between the prefetch loads)
        if constexpr (LIMBS && BM < 128 && TW == 32) __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (LIMBS) __syncthreads();                           // ONE stage: every wave has read tile t, the stage is free
    if constexpr (FLUSH) {
#pragma unroll
      for (int tt = 0; tt < 9; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { tot[tt][r] += acc[tt][r]; acc[tt][r] = 0.f; }
    }
    if (t + 1 < ntl) { W3_RETASK() W3_STORE(LIMBS ? 0 : cur ^ 1) }
    __syncthreads();
  }
#undef W3_LOAD
#undef W3_STORE
#undef W3_TASKS
#undef W3_RETASK
  if constexpr (FLUSH) {
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = tot[t];
  }

  WG3_REDUCE_TILES()
#endif
}

// ------------------------------------------------------------------------------------------------
// 3x3 on blk operands, no staging pass (gfx950: LDS-DMA + ds_read_b64_tr_b16).  The register-staged version of round 3 -- per thread
// and 64-pixel tile 8 x 16-byte loads, an 8 x 8 transposition (~100 VALU) and 8 LDS writes, a full memory round trip per tile behind
// one stage of prefetch -- bound those launches at ~1.4 us per tile and CU whatever the channel counts (a decoder
// level with 32 gate rows over 4 M pixels ran 10x over its HBM time).  Here the blk cells go from HBM to LDS as they are, by DMA
// (1 KB per wave instruction: 16 pixels x the 4 channel blocks of a 32-channel slab, [pixel][cb][8 ch] = 64 bytes per pixel), NR
// tiles deep, and the MFMA operands -- 8 consecutive pixels of one channel per lane -- are gathered by the transposing LDS read:
// within a 16-lane group, result element j of lane l is element l % 4 of the 8-byte chunk lane 4 j + l / 4 pointed at
// (tools/exp/tr16_probe.hip), so lane q of a group points at pixel q / 4, channels 4 (q % 4) .. + 3 of the group's 16 channels: the
// 32 lanes of a K half read 4 pixels x 64 bytes = 256 consecutive bytes (no bank conflict), a second read 4 pixels on completes
// the operand, and the 9 taps are 9 immediate offsets ((r PW + s) 64 bytes) off one per-lane base -- no VALU in the loop at all.
// Tile = TW x TH pixels (TW x TH / 16 K steps, dealt over the 4 / (BM / 32) wave copies of a row group); accumulators, split-K and
// the epilogue are those of wgrad3_bf16_body.
// ------------------------------------------------------------------------------------------------
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_p;
// The transposing reads are inline asm: behind the intrinsic (__builtin_amdgcn_ds_read_tr16_b64_*) hipcc waits vmcnt(0) before the first
// read of every tile -- for the DMA of the NEXT tile, issued a few instructions earlier -- and the ring degenerates to load-then-compute
// (measured: 2.9 us per 128-pixel tile and block whatever NR; plain ds_read_b64 in the same place gets no such wait).  The asm reads are
// invisible to the waitcnt pass, so their lgkmcnt is counted by hand: LDS returns in order, `s_waitcnt lgkmcnt(N)` = all but the N
// youngest reads have landed (scalar loads in flight can only make the wait longer).  The waits name the registers they guard as
// in/out operands so that no consumer is scheduled above them.
#define TR_READ(dst, addr, OFF) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory")
#define TR_WAIT8(N, a0, a1, b0, b1, b2, b3, b4, b5)                                                                \
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5) : "n"(N))
#define TR_WAITN(N) asm volatile("s_waitcnt lgkmcnt(%0)" : : "n"(N) : "memory")
#define TR_PIN(reg) asm volatile("" : "+v"(reg))        // (orders the consumers of `reg` behind the wait above: volatile asm keeps its order)
__device__ __forceinline__ bf16x8 tr_cat(const s16x4 lo, const s16x4 hi) {
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

template <int BM, int TW, int TH, int NR>
__device__ __forceinline__ void wgrad3_tr_body(const WgradBf16Args& p, const int bx, const int by) {
#if __HIP_DEVICE_COMPILE__
  using Geo = W3Ring<BM, TW, TH, NR>;
  constexpr int NK = Geo::NK, PW = Geo::PW, XPX = Geo::XPX, NA = Geo::NA, NX = Geo::NX;
  constexpr int C_DMA = Geo::C_DMA, ST_BYTES = Geo::ST_BYTES, X_OFF = Geo::X_OFF;
  constexpr int WGM = BM / 32, KSPW = 4 / WGM, NGG = NK / KSPW;
  static_assert(WGM * KSPW == 4 && NK % KSPW == 0, "config");
  char* const lds = wgb_stage_lds<Geo::LDS_BYTES, true>();

  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WGM, wk = wave / WGM;
  const int H = p.H, W = p.W, HW = H * W, Cs = p.Cs, Cout = p.Cout;
  const int co_t = bx % p.n_co_tiles, n_t = bx / p.n_co_tiles;
  const int co0 = co_t * BM, ci0 = n_t * 32;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int t_begin = by * p.tiles_per_split;
  const int t_end = min(t_begin + p.tiles_per_split, p.n_sp_tiles);
  if (t_begin >= t_end) return;

  // ---- loop-invariant part of this lane's share of a stage: instruction d = wave + 4 i moves pixels 16 (d % ..) + lane / 4 ----
  int d_y[C_DMA], d_x[C_DMA], d_cb[C_DMA];           // tile-local pixel (halo: -1), channel-block offset in cells; d_cb < 0: filler
  bool d_a[C_DMA];
#pragma unroll
  for (int i = 0; i < C_DMA; ++i) {
    const int d = wave + 4 * i;
    d_a[i] = d < NA;
    if (d < NA) {
      const int pa = 16 * (d % NK) + (lane >> 2);
      d_y[i] = pa / TW; d_x[i] = pa % TW;
      d_cb[i] = ((d / NK) * 4 + (lane & 3)) * HW;
    } else {
      const int pi = 16 * (d - NA) + (lane >> 2);
      d_y[i] = pi / PW - 1; d_x[i] = pi % PW - 1;
      d_cb[i] = (d < NA + NX && pi < XPX) ? (lane & 3) * HW : -1;
    }
  }
  const size_t a_img = (size_t)(Cout >> 3) * HW * 16, x_img = (size_t)(Cs >> 3) * HW * 16;
  const char* const a_base = (const char*)p.dy + (size_t)(co0 >> 3) * HW * 16;
  const char* const x_base = (const char*)p.x + (size_t)(ci0 >> 3) * HW * 16;
  const int a_len = ((Cout - co0) >> 3) * HW * 16, x_len = ((Cs - ci0) >> 3) * HW * 16;

  WgCursor cs(t_begin, tiles_x, tiles_y);            // (scalar; of the NEXT tile to fetch)
#define W3T_ISSUE(SLOT)                                                                                            \
  {                                                                                                                \
    const int y0 = cs.ty * TH, x0 = cs.tx * TW;                                                                    \
    const __amdgpu_buffer_rsrc_t ra_ = __builtin_amdgcn_make_buffer_rsrc((void*)(a_base + cs.tb * a_img), 0, a_len, 0x00020000); \
    const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc((void*)(x_base + cs.tb * x_img), 0, x_len, 0x00020000); \
    char* const sd = lds + (SLOT) * ST_BYTES + wave * 1024;                                                        \
    _Pragma("unroll") for (int i = 0; i < C_DMA; ++i) {                                                            \
      const int gy = y0 + d_y[i], gx = x0 + d_x[i];                                                                \
      const bool ok = d_cb[i] >= 0 && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;                    \
      const unsigned off = ok ? (unsigned)(d_cb[i] + gy * W + gx) * 16u : RSIS_OOB;                                \
      wg_dma(d_a[i], ra_, rx_, sd, i * 4096, off);                                                                \
    }                                                                                                              \
    cs.next(tiles_x, tiles_y);                                                                                     \
  }

  // ---- per-lane operand bases (bytes inside a stage) ----
  const int q16 = lane & 15, grp = lane >> 4;
  const int lane_c = (grp & 1) * 32 + (q16 & 3) * 8;               // byte of this lane's 4 channels inside the 64-byte pixel
  int aoff[NGG], xoff[NGG];
#pragma unroll
  for (int gg = 0; gg < NGG; ++gg) {
    const int pa = 16 * (gg * KSPW + wk) + 8 * hi + (q16 >> 2);
    aoff[gg] = wm * NK * 1024 + pa * 64 + lane_c;
    xoff[gg] = X_OFF + ((pa / TW) * PW + pa % TW) * 64 + lane_c;
  }

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  const int ntl = t_end - t_begin;
#pragma unroll
  for (int i = 0; i < NR - 1; ++i)
    if (i < ntl) W3T_ISSUE(i)
  for (int t = 0; t < ntl; ++t) {
    wg_ring_wait<NR, C_DMA>(t, ntl);
    __builtin_amdgcn_s_barrier();                     // tile t is in LDS (every wave's share); slot (t - 1) % NR is free
    if (t + NR - 1 < ntl) W3T_ISSUE((t + NR - 1) % NR)
    // K steps of this wave, software-pipelined over the LDS queue: the reads of (step, patch row r) are re-issued for the next step
    // right behind the 3 MFMAs that consumed row r, so that 14 reads (two rows + the next dy operand) are in flight under them
    const unsigned sb = lds0 + (t % NR) * ST_BYTES;
    s16x4 A[2][2], X[3][3][2];
#define W3T_READ_A(GG) { const unsigned aa = sb + aoff[GG]; TR_READ(A[(GG) & 1][0], aa, 0); TR_READ(A[(GG) & 1][1], aa, 256); }
#define W3T_READ_ROW(GG, R)                                                                                        \
  {                                                                                                                \
    const unsigned xa = sb + xoff[GG];                                                                             \
    TR_READ(X[R][0][0], xa, ((R) * PW + 0) * 64); TR_READ(X[R][0][1], xa, ((R) * PW + 0) * 64 + 256);              \
    TR_READ(X[R][1][0], xa, ((R) * PW + 1) * 64); TR_READ(X[R][1][1], xa, ((R) * PW + 1) * 64 + 256);              \
    TR_READ(X[R][2][0], xa, ((R) * PW + 2) * 64); TR_READ(X[R][2][1], xa, ((R) * PW + 2) * 64 + 256);              \
  }
#define W3T_ROW(GG, R, N)                                                                                          \
  {                                                                                                                \
    TR_WAIT8(N, A[(GG) & 1][0], A[(GG) & 1][1], X[R][0][0], X[R][0][1], X[R][1][0], X[R][1][1], X[R][2][0], X[R][2][1]); \
    const bf16x8 a = tr_cat(A[(GG) & 1][0], A[(GG) & 1][1]);                                                       \
    acc[(R) * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, tr_cat(X[R][0][0], X[R][0][1]), acc[(R) * 3 + 0], 0, 0, 0); \
    acc[(R) * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, tr_cat(X[R][1][0], X[R][1][1]), acc[(R) * 3 + 1], 0, 0, 0); \
    acc[(R) * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, tr_cat(X[R][2][0], X[R][2][1]), acc[(R) * 3 + 2], 0, 0, 0); \
  }
    W3T_READ_A(0) W3T_READ_ROW(0, 0) W3T_READ_ROW(0, 1) W3T_READ_ROW(0, 2)
#pragma unroll
    for (int gg = 0; gg < NGG; ++gg) {
      if (gg + 1 < NGG) {
        W3T_ROW(gg, 0, 12) W3T_READ_A(gg + 1) W3T_READ_ROW(gg + 1, 0)
        W3T_ROW(gg, 1, 14) W3T_READ_ROW(gg + 1, 1)
        W3T_ROW(gg, 2, 14) W3T_READ_ROW(gg + 1, 2)
      } else {
        W3T_ROW(gg, 0, 12) W3T_ROW(gg, 1, 6) W3T_ROW(gg, 2, 0)
      }
    }
#undef W3T_READ_A
#undef W3T_READ_ROW
#undef W3T_ROW
  }
#undef W3T_ISSUE
  __syncthreads();
  WG3_REDUCE_TILES()
#endif
}
// ------------------------------------------------------------------------------------------------
// 1x1 on blk operands, the same way (DMA ring of raw cells, transposing reads): D[co][ci] over BM x BN with 2 x 2 waves, a stage =
// TP consecutive pixels of the flattened map for the BM / 32 + BN / 32 channel slabs of the two operands; every wave walks all TP / 16
// K steps, the reads of step g + 1 in flight under the MFMAs of step g (two register sets, lgkmcnt counted by hand).
// ------------------------------------------------------------------------------------------------
template <int BM, int BN, int TP, int NR>
__device__ __forceinline__ void wgrad1_tr_body(const WgradBf16Args& p, const int bx, const int by) {
#if __HIP_DEVICE_COMPILE__
  using Geo = W1Ring<BM, BN, TP, NR>;
  constexpr int NK = Geo::NK, SA = Geo::SA, ND = Geo::ND, C_DMA = Geo::C_DMA, ST_BYTES = Geo::ST_BYTES, B_OFF = Geo::B_OFF;
  constexpr int WGM = 2, WGN = 2, TM = BM / WGM / 32, TN = BN / WGN / 32;
  constexpr int NRD = 2 * (TM + TN);                   // LDS reads per K step
  static_assert(TM >= 1 && TN >= 1 && NRD <= 15, "config");
  char* const lds = wgb_stage_lds<Geo::LDS_BYTES, true>();

  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int HW = p.W, Cs = p.Cs, Cout = p.Cout;        // (1x1: H = 1, W = the flattened map)
  const int co_t = bx % p.n_co_tiles, n_t = bx / p.n_co_tiles;
  const int co0 = co_t * BM, n0 = n_t * BN;
  const int tiles_x = (HW + TP - 1) / TP;
  const int t_begin = by * p.tiles_per_split;
  const int t_end = min(t_begin + p.tiles_per_split, p.n_sp_tiles);
  if (t_begin >= t_end) return;

  int d_px[C_DMA], d_cb[C_DMA];                        // pixel inside the tile; channel-block offset in cells (< 0: filler)
  bool d_a[C_DMA];
#pragma unroll
  for (int i = 0; i < C_DMA; ++i) {
    const int d = wave + 4 * i;
    d_a[i] = d < SA * NK;
    const int slab = d_a[i] ? d / NK : (d - SA * NK) / NK;
    d_px[i] = 16 * (d % NK) + (lane >> 2);
    d_cb[i] = d < ND ? (slab * 4 + (lane & 3)) * HW : -1;
  }
  const size_t a_img = (size_t)(Cout >> 3) * HW * 16, x_img = (size_t)(Cs >> 3) * HW * 16;
  const char* const a_base = (const char*)p.dy + (size_t)(co0 >> 3) * HW * 16;
  const char* const x_base = (const char*)p.x + (size_t)(n0 >> 3) * HW * 16;
  const int a_len = ((Cout - co0) >> 3) * HW * 16, x_len = ((Cs - n0) >> 3) * HW * 16;

  WgCursor cs(t_begin, tiles_x, 1);
#define W1T_ISSUE(SLOT)                                                                                            \
  {                                                                                                                \
    const int x0 = cs.tx * TP;                                                                                     \
    const __amdgpu_buffer_rsrc_t ra_ = __builtin_amdgcn_make_buffer_rsrc((void*)(a_base + cs.tb * a_img), 0, a_len, 0x00020000); \
    const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc((void*)(x_base + cs.tb * x_img), 0, x_len, 0x00020000); \
    char* const sd = lds + (SLOT) * ST_BYTES + wave * 1024;                                                        \
    _Pragma("unroll") for (int i = 0; i < C_DMA; ++i) {                                                            \
      const int gx = x0 + d_px[i];                                                                                 \
      const unsigned off = (d_cb[i] >= 0 && gx < HW) ? (unsigned)(d_cb[i] + gx) * 16u : RSIS_OOB;                  \
      wg_dma(d_a[i], ra_, rx_, sd, i * 4096, off);                                                                \
    }                                                                                                              \
    cs.next(tiles_x, 1);                                                                                           \
  }

  const int q16 = lane & 15, grp = lane >> 4;
  const unsigned lane_o = (8 * hi + (q16 >> 2)) * 64 + (grp & 1) * 32 + (q16 & 3) * 8;     // K half, pixel in the quad, channel quad
  const unsigned a_lane = wm * TM * NK * 1024 + lane_o, b_lane = B_OFF + wn * TN * NK * 1024 + lane_o;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  const int ntl = t_end - t_begin;
#pragma unroll
  for (int i = 0; i < NR - 1; ++i)
    if (i < ntl) W1T_ISSUE(i)
  for (int t = 0; t < ntl; ++t) {
    wg_ring_wait<NR, C_DMA>(t, ntl);
    __builtin_amdgcn_s_barrier();
    if (t + NR - 1 < ntl) W1T_ISSUE((t + NR - 1) % NR)
    const unsigned sa = lds0 + (t % NR) * ST_BYTES + a_lane, sbb = lds0 + (t % NR) * ST_BYTES + b_lane;
    s16x4 A[2][TM][2], B[2][TN][2];
#define W1T_READ(G)                                                                                                \
  {                                                                                                                \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                               \
      const unsigned aa = sa + i * NK * 1024;                                                                      \
      TR_READ(A[(G) & 1][i][0], aa, (G) * 1024); TR_READ(A[(G) & 1][i][1], aa, (G) * 1024 + 256);                  \
    }                                                                                                              \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                               \
      const unsigned ba = sbb + j * NK * 1024;                                                                     \
      TR_READ(B[(G) & 1][j][0], ba, (G) * 1024); TR_READ(B[(G) & 1][j][1], ba, (G) * 1024 + 256);                  \
    }                                                                                                              \
  }
    W1T_READ(0)
#pragma unroll
    for (int g = 0; g < NK; ++g) {
      if (g + 1 < NK) {
        if (g == 0) W1T_READ(1) else if (g == 1) W1T_READ(2) else if (g == 2) W1T_READ(3) else if (g == 3) W1T_READ(4)
        else if (g == 4) W1T_READ(5) else if (g == 5) W1T_READ(6) else W1T_READ(7)
      }
      // the reads of step g have landed once at most the NRD reads of step g + 1 are outstanding
      if (g + 1 < NK) { TR_WAITN(NRD); } else { TR_WAITN(0); }
#pragma unroll
      for (int i = 0; i < TM; ++i) { TR_PIN(A[g & 1][i][0]); TR_PIN(A[g & 1][i][1]); }
#pragma unroll
      for (int j = 0; j < TN; ++j) { TR_PIN(B[g & 1][j][0]); TR_PIN(B[g & 1][j][1]); }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_cat(A[g & 1][i][0], A[g & 1][i][1]), tr_cat(B[g & 1][j][0], B[g & 1][j][1]), acc[i][j], 0, 0, 0);
    }
#undef W1T_READ
  }
#undef W1T_ISSUE
  wg_atomic_tiles<TM, TN>(acc, p.dw, Cout, p.ldo, p.n_off, p.interleave_hid, co0 + wm * TM * 32 + 4 * hi, n0 + wn * TN * 32 + l31, Cs);
#endif
}
#ifndef W1T_TP
#define W1T_TP 64
#endif
constexpr int w1t_nr(int bm, int bn) { return (bm + bn) >= 256 ? 2 : 3; }

// tile height / ring depth of the (BM, TW) instantiations: the deepest tile whose ring fits 64 KB of static LDS, two blocks per CU
#ifndef W3T_TH_32_32      // (tuning builds override the three configurations that carry the step: -DW3T_TH_32_32=.. -DW3T_NR_32_32=.. ...)
#define W3T_TH_32_32 4
#define W3T_NR_32_32 2
#endif
#ifndef W3T_TH_64_32
#define W3T_TH_64_32 4
#define W3T_NR_64_32 2
#endif
#ifndef W3T_TH_64_16
#define W3T_TH_64_16 8
#define W3T_NR_64_16 2
#endif
constexpr int w3t_th(int bm, int tw) {
  return tw == 32 ? (bm == 128 ? 2 : (bm == 64 ? W3T_TH_64_32 : W3T_TH_32_32)) : (tw == 16 ? (bm == 128 ? 4 : (bm == 64 ? W3T_TH_64_16 : 8)) : 8);
}
constexpr int w3t_nr(int bm, int tw) {
  return tw == 32 ? (bm == 128 ? 2 : (bm == 64 ? W3T_NR_64_32 : W3T_NR_32_32)) : (tw == 16 ? (bm == 32 ? 3 : (bm == 64 ? W3T_NR_64_16 : 2)) : (bm == 128 ? 2 : 3));
}

// ------------------------------------------------------------------------------------------------
// 1x1: D[co][ci] = sum_px dy[co][px] x[ci][px]; block tile BM x BN, waves WGM x WGN, TM x TN MFMA tiles per wave.
// ------------------------------------------------------------------------------------------------
// LIMBS = 1: as in wgrad3_bf16_body -- three limb planes of the stage, split once per staged element, ONE stage; per K16 step
// 3 (TM + TN) reads for 6 TM TN MFMAs, limb pair outermost.
template <int BM, int BN, int WGM, int WGN, int TW, int IN, int LIMBS = 0>
__device__ __forceinline__ void wgrad1_bf16_body(const WgradBf16Args& p, const int bx, const int by) {
#if __HIP_DEVICE_COMPILE__
  using Geo = W1Stage<BM, BN, LIMBS>;
  constexpr int TH = Geo::TP / TW, GPR = TW / 8, NG = Geo::NG, KSTEPS = Geo::KSTEPS;
  constexpr int ARS = Geo::ARS, A_BYTES = Geo::A_BYTES, ST_BYTES = Geo::ST_BYTES, NTA = Geo::NTA, NTB = Geo::NTB;
  constexpr int TM = BM / WGM / 32, TN = BN / WGN / 32, NPL = Geo::NPL, NPROD = LIMBS ? RSIS_LIMB_PRODUCTS : 1;
  static_assert(WGM * WGN == 4, "config");
  char* const lds = wgb_stage_lds<Geo::LDS_BYTES, LIMBS != 0>();

  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int H = p.H, W = p.W, HW = H * W, Cs = p.Cs, Cout = p.Cout;
  const int co_t = bx % p.n_co_tiles, n_t = bx / p.n_co_tiles;
  const int co0 = co_t * BM, n0 = n_t * BN;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int t_begin = by * p.tiles_per_split;
  const int t_end = min(t_begin + p.tiles_per_split, p.n_sp_tiles);
  if (t_begin >= t_end) return;

  int a_off[NTA], a_y[NTA], a_x[NTA], a_lds[NTA];
  wg_row_tasks<NTA, NG, GPR, ARS>(tid, co0, Cout, HW, W, a_off, a_y, a_x, a_lds);
  int b_off[NTB], b_y[NTB], b_x[NTB], b_lds[NTB];
  wg_row_tasks<NTB, NG, GPR, ARS>(tid, n0, Cs, HW, W, b_off, b_y, b_x, b_lds);
  const int a_base = (wm * TM * 32 + l31) * ARS + hi * 16;
  const int b_base = (wn * TN * 32 + l31) * ARS + hi * 16;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  WgCursor cs(t_begin, tiles_x, tiles_y);

  // LIMBS: every tile starts from zero accumulators, added to `tot` on the VALU (see wgrad3_bf16_body)
  [[maybe_unused]] f32x16 tot[LIMBS ? TM : 1][LIMBS ? TN : 1];
  if constexpr (LIMBS) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
  }

  Task8<IN == 1> ra[NTA], rb[NTB];
#define W1_LOAD()                                                                                                  \
  {                                                                                                                \
    const int y0 = cs.ty * TH, x0 = cs.tx * TW;                                                                          \
    const int tsc = y0 * W + x0;                                                                                   \
    const float* ab = p.dy + ((size_t)cs.tb * Cout + co0) * HW;                                                       \
    const __amdgpu_buffer_rsrc_t ra_ = __builtin_amdgcn_make_buffer_rsrc((void*)ab, 0, (Cout - co0) * HW * 4, 0x00020000); \
    _Pragma("unroll") for (int i = 0; i < NTA; ++i)                                                                \
      ra[i].load(ra_, a_off[i] + tsc, a_off[i] >= 0 && y0 + a_y[i] < H, x0 + a_x[i], W);                           \
    const float* xb = p.x + ((size_t)cs.tb * Cs + n0) * HW;                                                           \
    const __amdgpu_buffer_rsrc_t rb_ = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, (Cs - n0) * HW * 4, 0x00020000); \
    _Pragma("unroll") for (int i = 0; i < NTB; ++i)                                                                \
      rb[i].load(rb_, b_off[i] + tsc, b_off[i] >= 0 && y0 + b_y[i] < H, x0 + b_x[i], W);                           \
    cs.next(tiles_x, tiles_y);                                                                                     \
  }
#define W1_STORE(BUF)                                                                                              \
  {                                                                                                                \
    char* st = lds + (BUF) * ST_BYTES;                                                                             \
    if constexpr (LIMBS) {                                                                                         \
      u32x4 c[3];                                                                                                  \
      _Pragma("unroll") for (int i = 0; i < NTA; ++i) {                                                            \
        ra[i].limb_cells(c);                                                                                       \
        _Pragma("unroll") for (int l = 0; l < 3; ++l) *(u32x4*)(st + l * ST_BYTES + a_lds[i]) = c[l];              \
      }                                                                                                            \
      _Pragma("unroll") for (int i = 0; i < NTB; ++i) {                                                            \
        rb[i].limb_cells(c);                                                                                       \
        _Pragma("unroll") for (int l = 0; l < 3; ++l) *(u32x4*)(st + l * ST_BYTES + A_BYTES + b_lds[i]) = c[l];    \
      }                                                                                                            \
    } else {                                                                                                       \
      _Pragma("unroll") for (int i = 0; i < NTA; ++i) *(u32x4*)(st + a_lds[i]) = ra[i].cell();                     \
      _Pragma("unroll") for (int i = 0; i < NTB; ++i) *(u32x4*)(st + A_BYTES + b_lds[i]) = rb[i].cell();           \
    }                                                                                                              \
  }

  W1_LOAD() W1_STORE(0)
  __syncthreads();
  const int ntl = t_end - t_begin;
  for (int t = 0; t < ntl; ++t) {
    const int cur = LIMBS ? 0 : t & 1;
    if (t + 1 < ntl) W1_LOAD()
    const char* As = lds + cur * ST_BYTES + a_base;
    const char* Bs = lds + cur * ST_BYTES + A_BYTES + b_base;
#pragma unroll
    for (int g = 0; g < KSTEPS; ++g) {
      bf16x8 a[TM][NPL], b[TN][NPL];
#pragma unroll
      for (int l = 0; l < NPL; ++l) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i][l] = __builtin_bit_cast(bf16x8, *(const u32x4*)(As + l * ST_BYTES + i * 32 * ARS + g * 32));
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j][l] = __builtin_bit_cast(bf16x8, *(const u32x4*)(Bs + l * ST_BYTES + j * 32 * ARS + g * 32));
      }
#pragma unroll
      for (int q = 0; q < NPROD; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][LIMBS ? RSIS_LIMB_PA(q) : 0], b[j][LIMBS ? RSIS_LIMB_PB(q) : 0], acc[i][j], 0, 0, 0);
    }
    if constexpr (LIMBS) {
      __syncthreads();                                              // ONE stage: every wave has read tile t, the stage is free
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) { tot[i][j][r] += acc[i][j][r]; acc[i][j][r] = 0.f; }
    }
    if (t + 1 < ntl) W1_STORE(LIMBS ? 0 : cur ^ 1)
    __syncthreads();
  }
#undef W1_LOAD
#undef W1_STORE
  if constexpr (LIMBS) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = tot[i][j];
  }

  wg_atomic_tiles<TM, TN>(acc, p.dw, Cout, p.ldo, p.n_off, p.interleave_hid, co0 + wm * TM * 32 + 4 * hi, n0 + wn * TN * 32 + l31, Cs);
#endif
}

// ------------------------------------------------------------------------------------------------
// (the 3x3 kernels are compiled for TWO waves per SIMD -- `__launch_bounds__(256, 2)`: 9 accumulator tiles + staging registers came
//  to 150-190 VGPRs + 144 AGPRs, one wave per SIMD, and a loop whose every s_waitcnt / barrier stalls the whole SIMD; held to 256
//  registers (no AGPRs, at most 9 spilled in three fp32-operand variants) two blocks share a CU and the bf16 224^2 step went
//  19.66 -> 18.80 ms.  LDS allows two blocks in every variant.)
// The launch is a GROUP of jobs placed on the eight XCD lanes, a single weight gradient a group of one in the plain mode: wgrad_lanes.h.
struct WgbBlockIdx { __device__ __forceinline__ unsigned operator()() const { return blockIdx.x; } };      // wgb_find's block index
template <int BM, int TW, int IN>
__global__ __launch_bounds__(256, 2) void wgrad3_bf16_group_kernel(const WgradBf16Group g) {
  int j, tile, split;
  if (!wgb_find(g, WgbBlockIdx{}, j, tile, split)) return;
  wgrad3_bf16_body<BM, TW, IN>(g.job[j], tile, split);
}
// (the rings are dynamic LDS, up to 80 KB: two blocks per CU)
template <int BM, int TW, int TH, int NR>
__global__ __launch_bounds__(256, 2) void wgrad3_tr_group_kernel(const WgradBf16Group g) {
  int j, tile, split;
  if (!wgb_find(g, WgbBlockIdx{}, j, tile, split)) return;
  wgrad3_tr_body<BM, TW, TH, NR>(g.job[j], tile, split);
}
template <int BM, int BN, int TP, int NR>
__global__ __launch_bounds__(256, 2) void wgrad1_tr_group_kernel(const WgradBf16Group g) {
  int j, tile, split;
  if (!wgb_find(g, WgbBlockIdx{}, j, tile, split)) return;
  wgrad1_tr_body<BM, BN, TP, NR>(g.job[j], tile, split);
}
template <int BM, int BN, int WGM, int WGN, int TW, int IN>
__global__ __launch_bounds__(256) void wgrad1_bf16_group_kernel(const WgradBf16Group g) {
  int j, tile, split;
  if (!wgb_find(g, WgbBlockIdx{}, j, tile, split)) return;
  wgrad1_bf16_body<BM, BN, WGM, WGN, TW, IN>(g.job[j], tile, split);
}
// The staged limb kernels (LIMBS = 1 of the two register-staged bodies).  Their one stage of three limb planes is dynamic LDS:
// 3x3 52-103 KB (BM = 32 / 64: two blocks per CU; BM = 128: one, and with it the whole register file), 1x1 55-111 KB.
template <int BM, int TW, int IN>
__global__ __launch_bounds__(256, BM == 128 ? 1 : 2) void wgrad3_limb_group_kernel(const WgradBf16Group g) {
  int j, tile, split;
  if (!wgb_find(g, WgbBlockIdx{}, j, tile, split)) return;
  wgrad3_bf16_body<BM, TW, IN, 1>(g.job[j], tile, split);
}
template <int BM, int BN, int IN>
__global__ __launch_bounds__(256) void wgrad1_limb_group_kernel(const WgradBf16Group g) {
  int j, tile, split;
  if (!wgb_find(g, WgbBlockIdx{}, j, tile, split)) return;
  wgrad1_bf16_body<BM, BN, 2, 2, 64, IN, 1>(g.job[j], tile, split);
}

// The one launcher: DYN_LDS = Geo::DYN_BYTES of the kernel's body, the same constant the body lays its stage out by; sizes above
// 64 KB are an opt-in per kernel, made once.
typedef void (*WgbLaunchFn)(const WgradBf16Group&, int, hipStream_t);
template <auto Kernel, int DYN_LDS>
static void wgb_launch(const WgradBf16Group& g, int blocks, hipStream_t st) {
  if constexpr (DYN_LDS > 0) {
    static const hipError_t once = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DYN_LDS);
    (void)once;
  }
  hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(256), DYN_LDS, st, g);
}

// stride 1, "same" padding, 32-bit offsets inside one image slab
bool rsis_wgrad_bf16_supported(const WgradArgs& w, int ks) {
  if (!(ks == 1 || ks == 3) || w.stride != 1 || w.pad != ks / 2 || w.H != w.Ho || w.W != w.Wo) return false;
  if (w.Cout == 1) return false;          // conv_out: HBM-bound VALU kernel (conv_c1.hip)
  if (w.blk && ((w.Cout & 7) || (w.Cs & 7))) return false;
  const long img = (long)w.H * w.W * 4;
  return (long)w.Cout * img < (1L << 30) && (long)w.Cs * img < (1L << 30);
}

// ---- which fp32 jobs run on the staged limb kernels ----
// A pure function of the job.  Classes: 3x3 jobs whose source is a multiple of the 32-channel slab, by dy rows (Cout > 64: 0-2,
// Cout <= 64: 3-5) and by the tile width wgb_key gives the map (8 / 16 / 32: + 0 / 1 / 2); 1x1 bottleneck pairs (Cout >= 128 and
// Cs >= 128: 6) and the other 1x1 jobs with Cout > 32 (7).  Maps that the 64-pixel tile does not divide, 3x3 sources that fill a
// slab badly (the 8- / 16- / 24-channel decoder sources) and Cout <= 32 1x1 jobs have no class: unmeasured, they stay where they are.
static int wgl_class(const WgradArgs& w, int ks) {
  if (ks == 3) {
    const int twi = w.W > 16 ? 2 : (w.W > 8 ? 1 : 0), tw = 8 << twi;
    if (w.Cs % 32 || w.W % tw || w.H % (64 / tw)) return -1;
    return (w.Cout > 64 ? 0 : 3) + twi;
  }
  if ((w.H * w.W) % 64 || w.Cout <= 32) return -1;
  return w.Cout >= 128 && w.Cs >= 128 ? 6 : 7;
}
// the table: one bit per class, set only where both runs of the 256 x 256 training step with the class on the staged kernels gave a
// lower sum over all weight-gradient launches than both runs without it (profiles/r11_a_wgrad_staged_per_class.txt, NOTES (85)):
//   5 (Cout <= 64 on 32-wide tiles: layer 1 and the decoder's 64^2 / 32^2 sources)   7.47-7.49 ms against 7.60-7.64, 7.18-7.21 against 7.29-7.39
//   2 (Cout > 64 on 32-wide tiles: layer 2)   a tie on its own (7.60 / 7.60 against 7.60-7.64), 7.40-7.44 on top of class 5 against
//     7.47-7.49 without it: the two classes share one launch of the 64-row instantiation
// Measured slower and off: 0 (8-wide, +0.2 ms), 1 (16-wide: layer 3, +0.25 ms -- the 64-row kernel is at the register-split loop's
// time there, the 128-row one behind it), 6 (+1.3 ms) and 7 (+0.1 ms): the 1x1 stage splits only half as many values as the
// register-split loop and pays for it with one block per CU.  3 and 4: the step has no such job, unmeasured.
static unsigned wgl_class_mask() { return 1u << 5 | 1u << 2; }
// RSIS_WGRAD_LIMBS, read once (conv_wgrad_tiled.hip reads `0` and `all`): unset = the table; 0 / all / reg = no staged class (the f32
// loop / the register-split loop everywhere / the tables of conv_wgrad_tiled.hip alone); staged = every job rsis_wgrad_bf16_supported
// accepts, in deterministic mode too, and -1 (the caller returns RSIS_ERR_UNSUPPORTED) for a job it does not.
int rsis_wgrad_staged_limbs(const WgradArgs& w, int ks) {
  static const int mode = [] {
    const char* e = getenv("RSIS_WGRAD_LIMBS");
    if (!e || !e[0]) return 0;
    return strcmp(e, "staged") == 0 ? 2 : 1;
  }();
  if (mode == 2) return rsis_wgrad_bf16_supported(w, ks) ? 1 : -1;
  if (mode == 1 || rsis_deterministic() || !rsis_wgrad_bf16_supported(w, ks)) return 0;      // (deterministic mode: the parent's routing, bit for bit)
  const int cls = wgl_class(w, ks);
  return cls >= 0 && ((wgl_class_mask() >> cls) & 1u);
}

// ---- launch (host side): jobs bucketed by kernel instantiation ----
// The instantiation of a job -- the ONE statement of the rule, for a job launched on its own and for a job of a group alike.
//   3x3: the widest 64-pixel tile the map fills; 64 dy rows per block unless the patch side is deep: half the splits (= half the
//   atomics) of the 128-row tile for 20 % more operand reads (128 -> 128 @28^2: 51 -> 36 us, 256 -> 256 @14^2: 62 -> 59 us;
//   1024 -> 128 @14^2: 92 -> 101 us, kept at 128).
//   1x1: the reduction runs over the flattened map (the H*W pixels of a channel are contiguous; the caller has set W = H * W, H = 1),
//   64 pixels per tile: whole 16-byte loads whenever H*W % 4 == 0.  Tiled in 2-D the 14-pixel rows of the 224 x 224 pyramid went
//   dword by dword, 4x the VMEM instructions, and the texture-address rate -- not HBM -- bound the loop (256 -> 1024 @14^2: 43 -> 29 us).
struct WgbKey { int ks, bm, bn, tw, v4, th, limbs; };
static WgbKey wgb_key(const WgradBf16Args& a, int ks, int limbs) {
  WgbKey k = {ks, 0, 0, 0, 0, 0, a.blk ? 0 : limbs};      // limbs: an fp32 job on the staged limb kernels (LIMBS = 1 of the staged bodies)
  if (ks == 3) {
    k.tw = a.W > 16 ? 32 : (a.W > 8 ? 16 : 8);
    k.bm = a.Cout <= 32 ? 32 : ((a.Cout <= 64 || a.Cs <= 512) ? 64 : 128);
    k.bn = 32;
  } else {
    k.tw = a.blk ? W1T_TP : 64;
    k.bm = a.Cout <= 64 ? 64 : 128;
    k.bn = a.Cs <= 64 ? 64 : 128;
  }
  k.v4 = a.blk ? 2 : (a.W % 4 == 0 ? 1 : 0);      // the IN template argument (2: blk operands -> the DMA kernels)
  k.th = ks == 3 ? (a.blk ? w3t_th(k.bm, k.tw) : 64 / k.tw) : (a.blk ? 1 : 64 / k.tw);      // tile height (blk 3x3: the DMA kernel's tile)
  return k;
}
static inline bool wgb_same(const WgbKey& a, const WgbKey& b) { return a.ks == b.ks && a.bm == b.bm && a.bn == b.bn && a.tw == b.tw && a.v4 == b.v4 && a.limbs == b.limbs; }

// the kernel and the geometry of a key
#define WGB3(BMv, TWv)                                                                                             \
  if (k.bm == BMv && k.tw == TWv) {                                                                                \
    using Ring = W3Ring<BMv, TWv, w3t_th(BMv, TWv), w3t_nr(BMv, TWv)>;                                             \
    if (k.limbs) return k.v4 == 1 ? wgb_launch<wgrad3_limb_group_kernel<BMv, TWv, 1>, W3Stage<BMv, TWv, 1>::DYN_BYTES> \
                                  : wgb_launch<wgrad3_limb_group_kernel<BMv, TWv, 0>, W3Stage<BMv, TWv, 1>::DYN_BYTES>; \
    if (k.v4 == 2) return wgb_launch<wgrad3_tr_group_kernel<BMv, TWv, w3t_th(BMv, TWv), w3t_nr(BMv, TWv)>, Ring::DYN_BYTES>; \
    return k.v4 == 1 ? wgb_launch<wgrad3_bf16_group_kernel<BMv, TWv, 1>, W3Stage<BMv, TWv, 0>::DYN_BYTES>          \
                     : wgb_launch<wgrad3_bf16_group_kernel<BMv, TWv, 0>, W3Stage<BMv, TWv, 0>::DYN_BYTES>;         \
  }
#define WGB1(BMv, BNv)                                                                                             \
  if (k.bm == BMv && k.bn == BNv) {                                                                                \
    using Ring = W1Ring<BMv, BNv, W1T_TP, w1t_nr(BMv, BNv)>;                                                       \
    if (k.limbs) return k.v4 == 1 ? wgb_launch<wgrad1_limb_group_kernel<BMv, BNv, 1>, W1Stage<BMv, BNv, 1>::DYN_BYTES> \
                                  : wgb_launch<wgrad1_limb_group_kernel<BMv, BNv, 0>, W1Stage<BMv, BNv, 1>::DYN_BYTES>; \
    if (k.v4 == 2) return wgb_launch<wgrad1_tr_group_kernel<BMv, BNv, W1T_TP, w1t_nr(BMv, BNv)>, Ring::DYN_BYTES>; \
    return k.v4 == 1 ? wgb_launch<wgrad1_bf16_group_kernel<BMv, BNv, 2, 2, 64, 1>, W1Stage<BMv, BNv, 0>::DYN_BYTES> \
                     : wgb_launch<wgrad1_bf16_group_kernel<BMv, BNv, 2, 2, 64, 0>, W1Stage<BMv, BNv, 0>::DYN_BYTES>; \
  }
static WgbLaunchFn wgb_launcher(const WgbKey& k) {
  if (k.ks == 3) {
    WGB3(32, 32) WGB3(64, 32) WGB3(128, 32) WGB3(32, 16) WGB3(64, 16) WGB3(128, 16) WGB3(32, 8) WGB3(64, 8) WGB3(128, 8)
  } else {
    WGB1(64, 64) WGB1(64, 128) WGB1(128, 64) WGB1(128, 128)
  }
  return nullptr;
}
#undef WGB3
#undef WGB1
// Count tiles, plan, launch (wgrad_lanes.h).  `alone`: ONE job that rsis_launch_conv_wgrad_bf16 launches on its own -- split_plan,
// plain mode; otherwise XCD lanes, in as many launches as the group's tables need.
static int wgb_launch_bucket(WgradBf16Args* jobs, int n, const WgbKey& k, bool alone, hipStream_t st) {
  const WgbLaunchFn launch = wgb_launcher(k);
  if (!launch) return RSIS_ERR_ARG;
  const long total = wgb_count_tiles(jobs, n, k.bm, k.bn, k.tw, k.th);
  static const int env_tb = getenv("RSIS_WGB_GROUP_BLOCKS") ? atoi(getenv("RSIS_WGB_GROUP_BLOCKS")) : 0;     // tuning knob
  // (swept at the bench geometry, 224^2 / batch 32, with two blocks per CU resident: 640 18.77 ms per step, 768 18.51, 896 18.43,
  //  1024 18.79, 1280 18.53, 1536 18.52, 1792 18.52 -- twice each, reproducible to 0.02; 1024 happens to cut the layer-3 jobs badly)
  const long target_blocks = env_tb > 0 ? env_tb : 896;
  WgradBf16Group g;
  for (int j0 = 0; j0 < n;) {
    const WgbPlan pl = alone ? wgb_plan_alone(g, jobs[j0], rsis_deterministic())
                             : wgb_plan_lanes(g, jobs + j0, n - j0, total, target_blocks, rsis_deterministic());
    launch(g, pl.blocks, st);
    if (rsis_check_launch() != RSIS_OK) return RSIS_ERR_LAUNCH;
    j0 += pl.jobs;
  }
  return RSIS_OK;
}

// n weight gradients that rsis_wgrad_bf16_supported accepts, all with the same kernel size
static int wgb_launch_jobs(const WgradArgs* w, int n, int ks, bool alone, hipStream_t st) {
  if (n < 1) return RSIS_OK;
  WgradBf16Args* all = (WgradBf16Args*)malloc(sizeof(WgradBf16Args) * n * 2);
  WgbKey* key = (WgbKey*)malloc(sizeof(WgbKey) * n);
  if (!all || !key) { free(all); free(key); return RSIS_ERR_LAUNCH; }
  WgradBf16Args* bucket = all + n;
  for (int j = 0; j < n; ++j) {
    WgradBf16Args a = {};
    a.dy = w[j].dy; a.x = w[j].x; a.dw = w[j].dw; a.B = w[j].B; a.Cs = w[j].Cs; a.H = w[j].H; a.W = w[j].W; a.Cout = w[j].Cout;
    a.ldo = w[j].ldo; a.n_off = w[j].n_off; a.interleave_hid = (short)w[j].interleave_hid; a.blk = (short)w[j].blk;
    if (ks == 1) { a.W = w[j].H * w[j].W; a.H = 1; }      // 1x1: the flattened map
    all[j] = a;
    key[j] = wgb_key(a, ks, w[j].limbs);
  }
  int rc = RSIS_OK;
  for (int j = 0; j < n && rc == RSIS_OK; ++j) {
    if (key[j].ks < 0) continue;
    const WgbKey k = key[j];
    int m = 0;
    for (int i = j; i < n; ++i)
      if (key[i].ks >= 0 && wgb_same(key[i], k)) { bucket[m++] = all[i]; key[i].ks = -1; }
    rc = wgb_launch_bucket(bucket, m, k, alone, st);
  }
  free(all); free(key);
  return rc;
}

int rsis_launch_conv_wgrad_bf16_group(const WgradArgs* w, int n, int ks, hipStream_t st) { return wgb_launch_jobs(w, n, ks, false, st); }
// one weight gradient in a launch of its own: a group of one job, plain mode
int rsis_launch_conv_wgrad_bf16(const WgradArgs& w, int ks, hipStream_t st) { return wgb_launch_jobs(&w, 1, ks, true, st); }
