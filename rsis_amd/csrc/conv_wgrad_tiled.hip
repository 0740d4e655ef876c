// Weight gradient of the stride-1 "same" convolutions (3x3/p1 and 1x1/p0) for gfx950 on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32), NCHW fp32, fed entirely by the LDS-DMA:
//     dW[co][ci][r][s] += sum_{b,y,x} dy[b][co][y][x] * x[b][ci][y+r-pad][x+s-pad]
// (autograd of nn.Conv2d in reference src/modules/clstm.py:17,44 -- the ConvLSTM gates, time-batched over T*B images --
//  model.py:43-47 and the 1x1 / 3x3 convs of the torchvision bottlenecks).
//
// GEMM view D[co][n], n = ci*ks*ks + rs (the reference's weight layout, so the result is accumulated straight into dW),
// the PIXELS are the reduction axis.  A block owns a BM x BN tile of D and walks a range of 8 x TH spatial tiles
// (split-K over tiles and images, fp32 atomics at the end).  Per spatial tile it copies into LDS, with
// `buffer_load ... lds` only (no staging registers, no ds_write pass, double buffered):
//   * the dy tile  As[BM][TP]  as float4 runs along W.  Row r keeps its 16-byte group G at slot G ^ (r & 7): the LDS image
//     stays lane-linear for the DMA (the swizzle is applied to the SOURCE offset) and the MFMA A operand of lane (r, h) is
//     ONE conflict-free ds_read_b128 per tile row y: group 2y+h = pixels (y, 4h..4h+3).  The K index of the MFMA is only
//     a summation index, so "lanes 0-31 take pixels x=0..3, lanes 32-63 take x=4..7 of row y" is as good as any order,
//     provided B uses the same one;
//   * 3x3: the input patch WITH halo  Xs[CI_P][TH+2][10]  as dwords (each input element once instead of 9 times; halo
//     outside the image gets an out-of-range offset, which the buffer descriptor turns into zeros).  The B operand of lane
//     n = (ci, r, s) is Xs[base(n) + 4h + y*10 + e]: a bare ds_read_b32 with an immediate offset;
//   * 1x1: the x tile Bs[BN][TP], same layout / same reads as dy.
// Per MFMA the wave issues <= 1 ds_read_b32 and 1/8..1/4 ds_read_b128; the DMA costs ~15 VMEM + ~25 VALU per thread per
// tile (128 MFMAs per wave for 3x3).  The spatial tile is as wide as the map allows (32x2 / 16x4 / 8x8 pixels for 3x3,
// 32x1 / 16x2 / 8x4 for 1x1) so that dy / x rows are read as full 128-byte lines; maps that no tile shape divides use
// conv_wgrad.hip.
//
// LIMB = 1 (the same kernels, another MFMA loop): the products run on v_mfma_f32_32x32x16_bf16.  The operands stay fp32 in LDS as the
// DMA lands them; after the ds_reads that exist anyway every value is split IN REGISTERS into three bf16 limbs whose sum is the value
// bit for bit (limb_split.h: by truncation; non-finite inputs give non-finite results, not necessarily of the same kind), and the
// limb pairs (i, j) with i + j <= 2 -- the six products of weight >= 2^-16, each exact in the fp32 accumulator's product -- replace
// the eight 64-cycle f32 MFMAs of a 16-pixel k-step by six 32-cycle ones.  Two consecutive step blocks g, g + 1 make one K16 step:
// lane (r, h) uses the 4 + 4 pixels it already reads as elements j = 0..7 of its k = 8h + j fragment, A and B alike.  Which tile
// configurations take this loop is a measured table (wg_limb_mask); RSIS_WGRAD_LIMBS=0 puts every job back on the f32 loop.
// (A second limb path splits every element once, when it is staged: LIMBS = 1 of conv_wgrad_bf16.hip.  Jobs its table selects
//  never reach this file; RSIS_WGRAD_LIMBS=reg keeps them here, =staged sends every job there -- see that file's header.)
//
// One launch path: conv_wgrad_tiled_group_kernel.  A single weight gradient is a group of one job; what differs between a job on its
// own and a group is the split plan (tiled_split_plan), nothing else.
#include "common.h"
#include "launchers.h"
#include "limb_split.h"
#include "wgrad_block_order.h"
#include "wgrad_parts.h"
#include <stdlib.h>
#include <string.h>


// limb pairs (A limb, B limb) of one K16 step, smallest weight first.  The first WG_LIMB_PRODUCTS are issued: 6 = the pairs with
// i + j <= 2; 9 would be the exact product.  (RSIS_LIMB_PA / PB of limb_split.h issue the same six in ANOTHER order, for the staged
// kernels' register budget; the order is the bits of a dW, so the two lists stay apart on purpose.)
#define WG_LIMB_PRODUCTS 6
[[maybe_unused]] __device__ constexpr int wg_limb_pa[9] = {2, 1, 0, 1, 0, 0, 2, 1, 2};
[[maybe_unused]] __device__ constexpr int wg_limb_pb[9] = {0, 1, 2, 0, 1, 0, 1, 2, 2};

// eight fp32 values (k = 0..7 of a lane's fragment) -> three bf16x8 limb fragments; element 2m sits in the low half of dword m
__device__ __forceinline__ void wg_limb_pack8(const float (&v)[8], bf16x8 (&out)[3]) {
  u32x4 q[3];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    float lo[3], hi[3];
    rsis_limb_split3(v[2 * m], lo[0], lo[1], lo[2]);
    rsis_limb_split3(v[2 * m + 1], hi[0], hi[1], hi[2]);
    // (limb 0 is packed from v itself: the permute takes the high halves, the mask is only needed for the residual)
    q[0][m] = __builtin_amdgcn_perm(__float_as_uint(v[2 * m + 1]), __float_as_uint(v[2 * m]), 0x07060302u);
    q[1][m] = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(lo[1]), 0x07060302u);
    q[2][m] = __builtin_amdgcn_perm(__float_as_uint(hi[2]), __float_as_uint(lo[2]), 0x07060302u);
  }
#pragma unroll
  for (int l = 0; l < 3; ++l) out[l] = __builtin_bit_cast(bf16x8, q[l]);
}

struct WgradTiledArgs {
  const float* dy;   // [B][CoutDy][H][W]
  const float* x;    // [B][Cs][H][W]
  float* dw;         // [Cout][ldo]
  int B, Cs, H, W, Cout;
  int ldo, n_off, interleave_hid;
  int n_co_tiles, n_n_tiles, n_sp_tiles, tiles_per_split;
};

// KSP = 2: the block's four waves form a WGM x WGN grid TWICE; the two copies take alternate halves of every stage's reduction
// depth and both add their partial tile with the (already atomic) epilogue -- lets a 32-row tile be only 64 columns wide.
// RAG: maps that no tile shape divides (the 7 / 14 / 28-pixel pyramid of 224 x 224 inputs).  The dy tile (and the x tile of a 1x1) then
// goes dword by dword -- four DMA instructions where the aligned map needs one dwordx4 -- so that every element carries its own
// "beyond the map" test: an element of the last tile column / row whose pixel lies outside gets an out-of-range offset and lands as
// 0.  The MFMA loop is unchanged (zeros add nothing); the tile grid rounds up.  RAG = 2: the map width is a multiple of 4 (28-pixel maps;
// every 1x1 whose H * W is, since a 1x1 may walk the FLATTENED map): a dwordx4 group is inside or outside as a whole, so the one
// DMA per group stays and only carries the two flag bits.
template <int BM, int BN, int WGM, int WGN, int KS, int TW, int KSP = 1, int RAG = 0, int LIMB = 0>
__device__ __forceinline__ void wgrad_tiled_body(const WgradTiledArgs& p, const int bx, const int by) {
#if __HIP_DEVICE_COMPILE__   // (the host pass only needs the launch stub; the buffer-resource builtins do not exist there)
  constexpr int TM = BM / WGM / 32, TN = BN / WGN / 32;
  constexpr int KK = KS * KS, HALO = KS / 2;
  constexpr int TP = KS == 1 ? 32 : 64;       // pixels per spatial tile = reduction depth per LDS stage
  constexpr int TH = TP / TW;                 // tile = TW x TH pixels: 32x2 / 16x4 / 8x8 (3x3), 32x1 / 16x2 / 8x4 (1x1)
  constexpr int NG = TP / 4;                  // 16-byte groups per dy row
  constexpr int GPR = TW / 4;                 // groups per tile row
  constexpr int PW = TW + 2 * HALO, PH = TH + 2 * HALO, IMS = PW * PH;
  constexpr int CI_P = KS == 1 ? BN : (BN + KK - 2) / KK + 1;   // input channels whose taps cover BN consecutive n
  constexpr int AS = BM * TP;                                   // floats per dy stage
  constexpr int XS = KS == 1 ? BN * TP : (CI_P * IMS + 255) / 256 * 256;
  constexpr int NA = BM * NG / 256;           // dwordx4 DMA per thread per tile (dy)
  constexpr int NB4 = KS == 1 ? BN * NG / 256 : 0;   // dwordx4 DMA per thread per tile (x, 1x1)
  constexpr int NB1 = KS == 1 ? 0 : XS / 256;        // dword DMA per thread per tile (x patch, 3x3)
  static_assert(WGM * WGN * KSP == 4 && (BM * NG) % 256 == 0 && (KS == 3 || (BN * NG) % 256 == 0) && (NG / 2) % KSP == 0 && (NG / 2 / KSP) % 2 == 0, "config");

  __shared__ __attribute__((aligned(16))) float lds[2 * (AS + XS)];
  float* const As0 = lds;
  float* const Xs0 = lds + 2 * AS;

  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wave / (WGM * WGN), wm = (wave % (WGM * WGN)) / WGN, wn = wave % WGN;
  const int H = p.H, W = p.W, HW = H * W, Cs = p.Cs, Cout = p.Cout;
  const int co_t = bx % p.n_co_tiles, n_t = bx / p.n_co_tiles;
  const int co0 = co_t * BM, n0 = n_t * BN;
  const int ci0 = n0 / KK;                     // first input channel of this block's patch / x tile
  const int Nn = Cs * KK;
  const int tiles_x = RAG ? (W + TW - 1) / TW : W / TW, tiles_y = RAG ? (H + TH - 1) / TH : H / TH;
  const int rx = W - (tiles_x - 1) * TW, ry = H - (tiles_y - 1) * TH;      // valid columns / rows of the last tile column / row
  const int t_begin = by * p.tiles_per_split;
  const int t_end = min(t_begin + p.tiles_per_split, p.n_sp_tiles);
  if (t_begin >= t_end) return;

  // ---- loop-invariant DMA offsets (bytes, relative to the tile's scalar base) ----
  unsigned voa[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int idx = tid + i * 256;
    const int row = idx / NG, sl = idx % NG;
    const int G = (sl & ~7) | ((sl & 7) ^ (row & 7));     // group held by this slot
    const int y = G / GPR, x4 = G % GPR;
    voa[i] = co0 + row < Cout ? ((unsigned)((co0 + row) * HW + y * W + x4 * 4) * 4u) | (RAG == 2 && x4 * 4 >= rx ? 1u : 0u) | (RAG == 2 && y >= ry ? 2u : 0u) : RSIS_OOB;
  }
  // RAG: dword DMA k of the dy tile moves LDS floats k * 256 + tid = element e of the dwordx4 slot (k * 256 + tid) / 4; bits 0 / 1 of
  // the offset (a multiple of 4) flag "column >= rx" / "row >= ry": outside the map in the last tile column / row
  unsigned voa1[RAG == 1 ? 4 * NA : 1];
  unsigned vob1r[RAG == 1 && NB4 ? 4 * NB4 : 1];
  if constexpr (RAG == 1) {
#pragma unroll
    for (int k = 0; k < 4 * NA; ++k) {
      const int P = k * 256 + tid, idx = P >> 2, e = P & 3;
      const int row = idx / NG, sl = idx % NG;
      const int G = (sl & ~7) | ((sl & 7) ^ (row & 7));
      const int y = G / GPR, x = (G % GPR) * 4 + e;
      voa1[k] = co0 + row < Cout ? ((unsigned)((co0 + row) * HW + y * W + x) * 4u) | (x >= rx ? 1u : 0u) | (y >= ry ? 2u : 0u) : RSIS_OOB;
    }
    if constexpr (KS == 1) {
#pragma unroll
      for (int k = 0; k < 4 * NB4; ++k) {
        const int P = k * 256 + tid, idx = P >> 2, e = P & 3;
        const int row = idx / NG, sl = idx % NG;
        const int G = (sl & ~7) | ((sl & 7) ^ (row & 7));
        const int y = G / GPR, x = (G % GPR) * 4 + e;
        vob1r[k] = n0 + row < Cs ? ((unsigned)((n0 + row) * HW + y * W + x) * 4u) | (x >= rx ? 1u : 0u) | (y >= ry ? 2u : 0u) : RSIS_OOB;
      }
    }
  }
  unsigned vob4[NB4 ? NB4 : 1];
  unsigned vob1[NB1 ? NB1 : 1];
  unsigned cls1[NB1 ? NB1 : 1];   // halo class of a patch element: 1 top row, 2 bottom row, 4 left column, 8 right column
  if constexpr (KS == 1) {
#pragma unroll
    for (int i = 0; i < NB4; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / NG, sl = idx % NG;
      const int G = (sl & ~7) | ((sl & 7) ^ (row & 7));
      const int y = G / GPR, x4 = G % GPR;
      vob4[i] = n0 + row < Cs ? ((unsigned)((n0 + row) * HW + y * W + x4 * 4) * 4u) | (RAG == 2 && x4 * 4 >= rx ? 1u : 0u) | (RAG == 2 && y >= ry ? 2u : 0u) : RSIS_OOB;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NB1; ++i) {
      const int e = tid + i * 256;
      const int cl = e / IMS, rem = e - cl * IMS;
      const int py = rem / PW, pxx = rem - py * PW;
      const bool ok = cl < CI_P && ci0 + cl < Cs;
      // relative to the element one row above / one column left of the tile origin in channel ci0 (+ (W+1)*4 so that it is >= 0)
      vob1[i] = ok ? (unsigned)(cl * HW + py * W + pxx) * 4u : RSIS_OOB;
      cls1[i] = (py == 0 ? 1u : 0u) | (py - 1 >= ry ? 2u : 0u) | (pxx == 0 ? 4u : 0u) | (pxx - 1 >= rx ? 8u : 0u);      // (aligned maps: ry = TH, rx = TW -- the halo ring)
    }
  }

  // ---- per-lane LDS read offsets ----
  // A (and 1x1 B): lanes 0-31 take group 2g, lanes 32-63 group 2g+1 of MFMA step block g; the group's slot in this lane's
  // row is (2g+h) ^ (row & 7), and row & 7 == l31 & 7 for every 32-row tile
  // (KSP == 2: this wave copy handles the step blocks g = 2 * gg + wk; their offsets live in per-wave registers)
  int sg[NG / 2 / KSP];
  int bo[NG / 2 / KSP];                        // 3x3: patch offset of the first pixel of step block g
#pragma unroll
  for (int gg = 0; gg < NG / 2 / KSP; ++gg) {
    const int g = gg * KSP + (KSP == 1 ? 0 : wk);
    sg[gg] = ((2 * g + hi) ^ (l31 & 7)) * 4;
    bo[gg] = KS == 1 ? 0 : (g / (TW / 8)) * PW + (g % (TW / 8)) * 8;
  }
  const int arow = (wm * TM * 32 + l31) * TP;
  int xb[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wn * TN * 32 + j * 32 + l31;          // column inside the block tile
    if constexpr (KS == 1) {
      xb[j] = nl * TP;
    } else {
      const int n = n0 + nl;
      const int cl = n / KK - ci0, rs = n - (n / KK) * KK;
      xb[j] = cl * IMS + (rs / KS) * PW + (rs % KS) + 4 * hi;
    }
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // scalar tile cursor
  int tb = t_begin / (tiles_x * tiles_y);
  int trem = t_begin - tb * (tiles_x * tiles_y);
  int ty = trem / tiles_x, tx = trem - ty * tiles_x;

#define WG_ISSUE(BUF)                                                                                          \
  {                                                                                                            \
    const int y0 = ty * TH, x0 = tx * TW;                                                                      \
    const float* ab = p.dy + ((size_t)tb * Cout * HW + y0 * W + x0);                                           \
    const __amdgpu_buffer_rsrc_t ra_ = __builtin_amdgcn_make_buffer_rsrc((void*)ab, 0, 0x7FFFFFF0, 0x00020000); \
    const unsigned lastm = (tx == tiles_x - 1 ? 1u : 0u) | (ty == tiles_y - 1 ? 2u : 0u);                      \
    if constexpr (RAG == 1) {                                                                                  \
      float* As = As0 + (BUF) * AS + wave * 64;                                                                \
      _Pragma("unroll") for (int k = 0; k < 4 * NA; ++k)                                                       \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (lds_vp_t)(As + k * 256), 4, (voa1[k] & lastm) ? RSIS_OOB : (voa1[k] & ~3u), 0, 0, 0); \
    } else {                                                                                                   \
      float* As = As0 + (BUF) * AS + wave * 256;                                                               \
      _Pragma("unroll") for (int i = 0; i < NA; ++i)                                                           \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (lds_vp_t)(As + i * 1024), 16,                           \
                                                 RAG == 2 ? ((voa[i] & lastm) ? RSIS_OOB : (voa[i] & ~3u)) : voa[i], 0, 0, 0); \
    }                                                                                                          \
    if constexpr (KS == 1) {                                                                                   \
      const float* bb = p.x + ((size_t)tb * Cs * HW + y0 * W + x0);                                            \
      const __amdgpu_buffer_rsrc_t rb_ = __builtin_amdgcn_make_buffer_rsrc((void*)bb, 0, 0x7FFFFFF0, 0x00020000); \
      if constexpr (RAG == 1) {                                                                                \
        float* Xs = Xs0 + (BUF) * XS + wave * 64;                                                              \
        _Pragma("unroll") for (int k = 0; k < 4 * NB4; ++k)                                                    \
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (lds_vp_t)(Xs + k * 256), 4, (vob1r[k] & lastm) ? RSIS_OOB : (vob1r[k] & ~3u), 0, 0, 0); \
      } else {                                                                                                 \
        float* Xs = Xs0 + (BUF) * XS + wave * 256;                                                             \
        _Pragma("unroll") for (int i = 0; i < NB4; ++i)                                                        \
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (lds_vp_t)(Xs + i * 1024), 16,                         \
                                                   RAG == 2 ? ((vob4[i] & lastm) ? RSIS_OOB : (vob4[i] & ~3u)) : vob4[i], 0, 0, 0); \
      }                                                                                                        \
    } else {                                                                                                   \
      const float* bb = p.x + (((size_t)tb * Cs + ci0) * HW + (y0 - 1) * W + (x0 - 1));                        \
      const __amdgpu_buffer_rsrc_t rb_ = __builtin_amdgcn_make_buffer_rsrc((void*)bb, 0, 0x7FFFFFF0, 0x00020000); \
      const unsigned edge = (y0 == 0 ? 1u : 0u) | (ty == tiles_y - 1 ? 2u : 0u) | (x0 == 0 ? 4u : 0u) | (tx == tiles_x - 1 ? 8u : 0u); \
      float* Xs = Xs0 + (BUF) * XS + wave * 64;                                                                \
      _Pragma("unroll") for (int i = 0; i < NB1; ++i) {                                                        \
        const unsigned vo = (cls1[i] & edge) ? RSIS_OOB : vob1[i];                                             \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (lds_vp_t)(Xs + i * 256), 4, vo, 0, 0, 0);               \
      }                                                                                                        \
    }                                                                                                          \
    if (++tx == tiles_x) { tx = 0; if (++ty == tiles_y) { ty = 0; ++tb; } }                                    \
  }
#define WG_LAND() __builtin_amdgcn_s_waitcnt(0x0F70);   /* vmcnt(0): this wave's DMA has landed in LDS */

  WG_ISSUE(0)
  WG_LAND()
  __syncthreads();
  const int ntl = t_end - t_begin;
  for (int t = 0; t < ntl; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntl) WG_ISSUE(cur ^ 1)   // stage cur^1 was last read before the barrier that ended step t-1
    {
      const float* As = As0 + cur * AS + arow;
      const float* Xs = Xs0 + cur * XS;
      if constexpr (LIMB) {
#pragma unroll
        for (int g = 0; g < NG / 2 / KSP; g += 2) {       // step blocks g, g + 1 = one K16 step
          bf16x8 al[TM][3], bl[TN][3];
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(As + i * 32 * TP + sg[g]);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(As + i * 32 * TP + sg[g + 1]);
            const float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            wg_limb_pack8(v, al[i]);
          }
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            float v[8];
            if constexpr (KS == 1) {
              const f32x4 b0 = *reinterpret_cast<const f32x4*>(Xs + xb[j] + sg[g]);
              const f32x4 b1 = *reinterpret_cast<const f32x4*>(Xs + xb[j] + sg[g + 1]);
#pragma unroll
              for (int e = 0; e < 4; ++e) { v[e] = b0[e]; v[4 + e] = b1[e]; }
            } else {
#pragma unroll
              for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  v[4 * u + e] = Xs[xb[j] + (KSP == 1 ? ((g + u) / (TW / 8)) * PW + ((g + u) % (TW / 8)) * 8 : bo[g + u]) + e];
            }
            wg_limb_pack8(v, bl[j]);
          }
          // limb pairs outside, tiles inside: consecutive MFMAs never share an accumulator (where TM * TN > 1)
#pragma unroll
          for (int q = 0; q < WG_LIMB_PRODUCTS; ++q)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i][wg_limb_pa[q]], bl[j][wg_limb_pb[q]], acc[i][j], 0, 0, 0);
        }
      } else
#pragma unroll
      for (int g = 0; g < NG / 2 / KSP; ++g) {
        f32x4 a4[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) a4[i] = *reinterpret_cast<const f32x4*>(As + i * 32 * TP + sg[g]);
        if constexpr (KS == 1) {
          f32x4 b4[TN];
#pragma unroll
          for (int j = 0; j < TN; ++j) b4[j] = *reinterpret_cast<const f32x4*>(Xs + xb[j] + sg[g]);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][e], b4[j][e], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float b[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Xs[xb[j] + (KSP == 1 ? (g / (TW / 8)) * PW + (g % (TW / 8)) * 8 : bo[g]) + e];   // pixel (y, x) of group 2g+h, element e
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][e], b[j], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
    WG_LAND()
    __syncthreads();
  }
#undef WG_ISSUE
#undef WG_LAND

  // ---- epilogue: fp32 atomics into dW (reference layout) ----
  wg_atomic_tiles<TM, TN>(acc, p.dw, Cout, p.ldo, p.n_off, p.interleave_hid, co0 + wm * TM * 32 + 4 * hi, n0 + wn * TN * 32 + l31, Nn);
#endif
}

// ---- the launch: the weight gradients of many layers in ONE grid (rsis_conv2d_wgrad_batch); a single weight gradient
// (rsis_conv2d_wgrad, and every job of the deterministic mode) is a group of one job.  A weight gradient is off the
// backward pass's critical path (nothing reads it before the optimizer step), so the training driver parks them and flushes
// them together: every launch costs ~15 us of ramp, prologue and drain whatever its size, and alone a layer has to split its
// pixel axis 8-32 ways to fill the chip -- each split a dW-sized pass of fp32 atomics -- while forty layers together fill it with
// one or two.  The jobs travel by value in the kernel arguments (no device-side table, nothing to keep alive under graph replay);
// logical block b belongs to the job whose [begin, end) range holds it and plays block (x, y) = (b' % tiles, b' / tiles) of that job
// -- for one job the order of a (tiles, splits) grid.  The hardware block index is first permuted (wgrad_block_order.h) so that the
// blocks one XCD runs are a contiguous range of logical blocks: consecutive dW tiles of a split share an x slab (the co tiles of one
// n tile) or a dy slab, and dealt round-robin they re-read it through eight different L2s.  The set of blocks, the split plan and the
// work per block do not change; with one contributor per dW tile (deterministic mode) neither do the bits. ----
#define RSIS_WG_MAXJ 48
struct WgradTiledGroup {
  int n;
  int xcd_order;          // 1: XCD-contiguous block order (grouped launches, wg_xcd_order); 0: the identity
  int begin[RSIS_WG_MAXJ + 1];
  WgradTiledArgs job[RSIS_WG_MAXJ];
};
static_assert(sizeof(WgradTiledGroup) <= 4000, "kernel arguments are limited to 4 KB");

template <int BM, int BN, int WGM, int WGN, int KS, int TW, int KSP = 1, int RAG = 0, int LIMB = 0>
__global__ __launch_bounds__(256) void conv_wgrad_tiled_group_kernel(const WgradTiledGroup g) {
  const int b = g.xcd_order ? rsis_xcd_logical_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  int lo = 0, hi = g.n - 1;
  while (lo < hi) {                       // last job whose begin <= b (uniform: scalar code)
    const int mid = (lo + hi + 1) >> 1;
    if (g.begin[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const WgradTiledArgs& p = g.job[lo];
  const int local = b - g.begin[lo];
  const int ntile = p.n_co_tiles * p.n_n_tiles;
  wgrad_tiled_body<BM, BN, WGM, WGN, KS, TW, KSP, RAG, LIMB>(p, local % ntile, local / ntile);
}

// ---- which tile configurations run the limb loop (LIMB = 1) ----
// One bit per tile configuration code of tiled_cfg_code (0 = 32x64 KSP 2, 1 = 32x128, 2 = 64x64, 3 = 64x128, 4 = 128x64, 5 = 128x128),
// per kernel size and tile width.  A bit is set where the grouped launch of that bucket in the 256 x 256 training step measured
// faster than the f32 loop by more than the run-to-run spread (profiles/r07_a_wgrad_limbs_per_config.txt, NOTES (73)): every 3x3
// bucket (0.66-0.93 of the f32 loop's time) and the 64x64 1x1 tile on 16- and 8-wide tiles (0.86 / 0.88); the 64x64 1x1 on 32-wide
// tiles (the 64- and 32-pixel maps) measured 1.20 and stays on the f32 loop.  The 128x128 1x1 tile of the grouped launches
// (wg_group_tile) measured 0.70-0.75 on all three tile widths (profiles/r09_a_wgrad_tiles_per_bucket.txt, NOTES (80)).  Buckets the
// step does not have, the ragged (RAG) ones among them, are unmeasured and stay off.
static unsigned wg_limb_mask(int ks, int tw) {
  if (ks == 3) return tw == 16 ? 0x3Fu : (tw == 8 ? 1u << 5 : 0u);
  return (tw == 16 || tw == 8 ? 1u << 2 : 0u) | 1u << 5;
}
// RSIS_WGRAD_LIMBS, read once: unset = the table; 0 = every job on the f32 loop (A/B, bisecting); all = every job on the limb loop
// (the per-configuration measurement and tests/test_gpu_wgrad_limbs.py); reg / staged (rsis_wgrad_staged_limbs) = the table here
static bool wg_use_limbs(int ks, int tw, int code, int rag) {
  static const int mode = [] {
    const char* e = getenv("RSIS_WGRAD_LIMBS");
    if (!e || !e[0]) return 0;
    if (e[0] == '0') return 1;
    return strcmp(e, "all") == 0 ? 2 : 0;
  }();
  if (mode) return mode == 2;
  return rag == 0 && ((wg_limb_mask(ks, tw) >> code) & 1u);
}

// ---- which buckets of a GROUPED launch run in the XCD-contiguous block order (wgrad_block_order.h) ----
// One bit per tile configuration code, per kernel size and tile width, like wg_limb_mask and from the same kind of measurement
// (profiles/r09_a_wgrad_tiles_per_bucket.txt, NOTES (80)).  A bit is set where every run in XCD order was faster than every run in
// hardware order: the 3x3 buckets 64 x 64 (0.88 of the hardware order's time) and 32 x 64 KSP 2 (0.93) on 16-wide tiles, the two 3x3
// buckets with 32 x 32 wave tiles and the highest fabric rates, and the 128 x 128 1x1 on 32-wide tiles (0.34-0.35 ms against 0.37-0.45).
// 128 x 64, 32 x 128 and 64 x 128 3x3 and the 128 x 128 1x1 on 16- / 8-wide tiles measured 0.95-0.99 with overlapping runs; the
// 128 x 128 3x3 did not move on 16-wide tiles and measured 1.14 on 8-wide ones; the 64 x 64 1x1 did not move.  Those, buckets the step
// does not have, and every launch of a single weight gradient (never measured) stay in hardware order.
static unsigned wg_xcd_mask(int ks, int tw) {
  if (ks == 3) return tw == 16 ? 0x5u : 0u;
  return tw == 32 ? 1u << 5 : 0u;
}
// RSIS_WGRAD_XCD, read once: unset = the table; 0 = every grouped launch in hardware order (A/B runs); all = every grouped launch
// in the XCD-contiguous order (tests/test_gpu_wgrad_tiles.py, the per-bucket measurement)
static int wg_xcd_order(int ks, int tw, int code, int rag) {
  static const int mode = [] {
    const char* e = getenv("RSIS_WGRAD_XCD");
    if (!e || !e[0]) return 0;
    if (e[0] == '0') return 1;
    return strcmp(e, "all") == 0 ? 2 : 0;
  }();
  if (mode) return mode == 2;
  return rag == 0 && ((wg_xcd_mask(ks, tw) >> code) & 1u);
}
// tile configuration code of a BM x BN block tile (the inverse of launch_group_code's switch)
static constexpr int tiled_code_of(int bm, int bn) { return bm == 32 ? (bn == 64 ? 0 : 1) : (bm == 64 ? (bn == 64 ? 2 : 3) : (bn == 64 ? 4 : 5)); }

// widest tile the map allows: full 128-byte lines of dy / x per tile row on the wide maps, whole rows on the narrow ones
static int tiled_tw(int H, int W, int ks) {
  const int tp = ks == 1 ? 32 : 64;
  // 3x3: the 32x2 tile's halo patch pushes the 128x128 configuration past 80 KB of LDS (1 block per CU); 16x4 measured equal
  // or better on every trunk / gate shape.  1x1 has no patch and prefers full 128-byte rows.
  for (int tw = ks == 1 ? 32 : 16; tw >= 8; tw >>= 1)
    if (W % tw == 0 && H % (tp / tw) == 0) return tw;
  return 0;
}
// ragged maps (RAG instantiations): the narrowest tile that is at least as wide as the map, or the widest one
static int tiled_tw_ragged(int W, int ks) {
  const int wide = ks == 1 ? 32 : 16;
  return W > 16 ? wide : (W > 8 ? 16 : 8);
}

// ---- launch (host side) ----
// tile configuration of a job: 0 = 32x64 (KSP 2), 1 = 32x128, 2 = 64x64, 3 = 64x128, 4 = 128x64, 5 = 128x128
// N = Cs * KS * KS columns: a 64-wide tile when that pads N less than the 128-wide one (N mod 128 in 1..64), e.g. the decoder's
// 16- and 32-channel sources (N = 144 / 288: 56 % / 75 % -> 75 % / 90 % useful MFMA columns)
// (deterministic mode: not the KSP = 2 tile -- its two wave copies both add into dW, in either order)
// 1x1: 64 x 64 tiles with two blocks per CU.  The split count -- and with it the dW-sized passes of fp32 atomics, which run at
// ~0.3 T atomics/s and were a third of these launches -- goes with slots / tiles: a quarter of the 128 x 128 tile's at twice
// its slots.  Measured on every 1x1 shape of the trunk at batch 32 (tools/exp/bf16_shape_sweep.py --dtype fp32): 47-54 -> 38-44 us.
static int tiled_cfg_code_single(const WgradTiledArgs& a, int ks) {
  const int nmod = (a.Cs * ks * ks) % 128;
  const bool narrow = nmod != 0 && nmod <= 64;
  if (ks == 1 && a.Cout > 32) return 2;
  if (a.Cout <= 32) return narrow && !rsis_deterministic() ? 0 : 1;
  if (a.Cout <= 64) return narrow ? 2 : 3;
  return narrow ? 4 : 5;
}

// ---- tile of a job inside a GROUPED launch on an aligned map ----
// The rule above was measured on single launches of the f32 loop, where a layer splits 8-32 ways and the atomics of the splits decide;
// in a group a layer splits 2-3 ways, and on the limb loop the 32 x 32 wave tiles (TM * TN = 1) of the small configurations pay twice
// the operand split per MFMA and re-read dy / x twice as often as the 128-wide ones.  The jobs for which a wider tile is a candidate
// fall into classes; which class takes it is a measured table (wg_group_tile), class by class like wg_limb_mask:
//   1x1, Cout > 32: class 1 = Cout >= 128 and Cs >= 128 (the bottleneck pairs of layers 2-4), class 0 = the rest; candidate 128 x 128
//   3x3 "narrow" N: class 0 / 1 / 2 = Cout <= 32 / <= 64 / above; candidate the 128-wide tile of the same BM (codes 1 / 3 / 5)
static int wg_job_class(const WgradTiledArgs& a, int ks) {
  if (ks == 1) return a.Cout <= 32 ? -1 : (a.Cout >= 128 && a.Cs >= 128 ? 1 : 0);
  const int nmod = (a.Cs * ks * ks) % 128;
  if (nmod == 0 || nmod > 64) return -1;
  return a.Cout <= 32 ? 0 : (a.Cout <= 64 ? 1 : 2);
}
static int wg_wide_code(int ks, int cls) { return ks == 1 ? 5 : 2 * cls + 1; }
// the table: tile configuration code of class `cls` on tw-wide spatial tiles, or -1 = the rule of the single launch.  An entry is
// set where the grouped launches of the 256 x 256 training step measured faster with it by more than the run-to-run spread
// (profiles/r09_a_wgrad_tiles_per_bucket.txt, NOTES (80)); classes the step does not have are unmeasured and stay on -1.
// Measured: the 1x1 bottleneck pairs on the 128 x 128 tile AND the limb loop 0.78 / 0.65 of the 64 x 64 tile's time on 16- / 32-wide
// tiles; on 8-wide tiles 0.92 in XCD order but 0.94-1.00 in hardware order, inside the spread: not taken.  On the f32 loop the same
// tile is 1.10 / 0.91 / 1.24 (16- / 32- / 8-wide): the gain is the halved operand split per MFMA, and wg_limb_mask carries the bit.
// 64 x 128 and 128 x 64 measured 0.85-0.87 on 16-wide tiles, behind it.  The other 1x1 jobs of the 32-wide bucket (Cout or Cs of 64)
// lose on it (1.76).  3x3: the Cout <= 64 class on 64 x 128 measured 0.96 in one step and 1.03 in another (not robust); the Cout <= 32
// class loses on 32 x 128 (1.05) and the Cout > 64 class on 128 x 128 (1.00 in hardware order, 1.16 in XCD order): all three stay.
static int wg_group_tile(int ks, int tw, int cls) {
  return ks == 1 && cls == 1 && (tw == 32 || tw == 16) ? 5 : -1;
}
// RSIS_WGRAD_TILES, read once: unset = the table; 0 = the single launch's rule everywhere; wide = every class on its candidate
// (tests/test_gpu_wgrad_tiles.py)
static int tiled_cfg_code(const WgradTiledArgs& a, int ks, int tw, bool grouped) {
  static const int mode = [] {
    const char* e = getenv("RSIS_WGRAD_TILES");
    if (!e || !e[0]) return 0;
    if (strcmp(e, "0") == 0) return 1;
    return strcmp(e, "wide") == 0 ? 2 : 0;
  }();
  const int single = tiled_cfg_code_single(a, ks);
  const int cls = wg_job_class(a, ks);
  if (!grouped || cls < 0 || mode == 1 || rsis_deterministic()) return single;
  const int code = mode == 2 ? wg_wide_code(ks, cls) : wg_group_tile(ks, tw, cls);
  return code < 0 ? single : code;
}

// ---- split plan: tiles_per_split of every job of one launch (n_co_tiles / n_n_tiles / n_sp_tiles are set).  Every split adds a
// full dW-sized pass of fp32 atomics, so a job is split as little as filling the chip allows; deterministic mode: no split, one
// block walks every spatial tile of its dW tile. ----
static void tiled_split_plan(WgradTiledArgs* jobs, int n, int ks, bool big_tile, bool alone, int rag) {
  if (alone && rag == 0) {
    // a launch of its own on an aligned map (rsis_conv2d_wgrad): fill the resident block slots (2 blocks per CU for the 128 x 128
    // tile, 3 otherwise) in one round, keeping >= 2 spatial tiles per split.  With the slots filled the atomics are
    // slots * BM * BN per launch whatever the layer (8.4 M for 128 x 128 tiles, ~20 us) -- a third of a 1x1 weight gradient's time
    // but < 10 % of a 3x3's.  Measured: 1x1 layers +15 % with one block per CU (half the splits), 3x3 layers lose up to 20 % (they
    // need the second block to hide the patch staging).
    WgradTiledArgs& a = jobs[0];
    const int ntile = a.n_co_tiles * a.n_n_tiles;
    const int slots = ks == 1 ? (big_tile ? 256 : 512) : 256 * (big_tile ? 2 : 3);
    int nsplit = ntile >= slots ? 1 : slots / ntile;
    if (nsplit > a.n_sp_tiles / 2) nsplit = a.n_sp_tiles / 2;
    if (nsplit < 1 || rsis_deterministic()) nsplit = 1;
    a.tiles_per_split = rsis_cdiv(a.n_sp_tiles, nsplit);
    return;
  }
  // a group -- and a ragged map launched on its own (rag != 0), which has always been planned as a group of one: equal work per block, every
  // block walks ~L >= 2 spatial tiles of its job; ~8 blocks per CU over the whole group keeps the tail short
  long total_iters = 0;
  for (int j = 0; j < n; ++j) total_iters += (long)jobs[j].n_co_tiles * jobs[j].n_n_tiles * jobs[j].n_sp_tiles;
  static const int env_tb = getenv("RSIS_WG_GROUP_BLOCKS") ? atoi(getenv("RSIS_WG_GROUP_BLOCKS")) : 0;     // tuning knob
  // (the target does not go with the tile area: the 128 x 128 1x1 buckets, four times the atomics per block of the 64 x 64 ones, measured
  //  1.04 / 1.06 / 0.98 at 1024 blocks against 2048 on 16- / 32- / 8-wide tiles -- NOTES (80))
  const long target_blocks = env_tb > 0 ? env_tb : 2048;
  long L = (total_iters + target_blocks - 1) / target_blocks;
  if (L < 2) L = 2;
  if (rsis_deterministic()) L = 1L << 40;
  for (int j = 0; j < n; ++j) {
    int nsplit = rsis_cdiv(jobs[j].n_sp_tiles, L);
    if (nsplit < 1) nsplit = 1;
    jobs[j].tiles_per_split = rsis_cdiv(jobs[j].n_sp_tiles, nsplit);
  }
}

// `alone`: the jobs are ONE job that rsis_launch_conv_wgrad_tiled launches on its own
template <int BM, int BN, int WGM, int WGN, int KS, int TW, int KSP = 1, int RAG = 0, int LIMB = 0>
static int launch_group_cfg(WgradTiledArgs* jobs, int n, bool alone, hipStream_t st) {
  constexpr int TH = (KS == 1 ? 32 : 64) / TW;
  for (int j = 0; j < n; ++j) {
    WgradTiledArgs& a = jobs[j];
    a.n_co_tiles = rsis_cdiv(a.Cout, BM);
    a.n_n_tiles = rsis_cdiv((long)a.Cs * KS * KS, BN);
    a.n_sp_tiles = RAG ? a.B * rsis_cdiv(a.H, TH) * rsis_cdiv(a.W, TW) : a.B * (a.H / TH) * (a.W / TW);
  }
  tiled_split_plan(jobs, n, KS, BM * BN >= 128 * 128, alone, RAG);
  for (int j0 = 0; j0 < n; j0 += RSIS_WG_MAXJ) {
    WgradTiledGroup g;
    g.xcd_order = !alone && wg_xcd_order(KS, TW, tiled_code_of(BM, BN), RAG);      // (a single launch keeps the hardware order)
    g.n = n - j0 < RSIS_WG_MAXJ ? n - j0 : RSIS_WG_MAXJ;
    int blocks = 0;
    for (int j = 0; j < g.n; ++j) {
      const WgradTiledArgs& a = jobs[j0 + j];
      g.begin[j] = blocks;
      g.job[j] = a;
      blocks += a.n_co_tiles * a.n_n_tiles * rsis_cdiv(a.n_sp_tiles, a.tiles_per_split);
    }
    g.begin[g.n] = blocks;
    hipLaunchKernelGGL((conv_wgrad_tiled_group_kernel<BM, BN, WGM, WGN, KS, TW, KSP, RAG, LIMB>), dim3(blocks), dim3(256), 0, st, g);
    if (rsis_check_launch() != RSIS_OK) return RSIS_ERR_LAUNCH;
  }
  return RSIS_OK;
}

template <int KS, int TW, int RAG, int LIMB>
static int launch_group_code(int code, WgradTiledArgs* jobs, int n, bool alone, hipStream_t st) {
  switch (code) {
    case 0: return launch_group_cfg<32, 64, 1, 2, KS, TW, 2, RAG, LIMB>(jobs, n, alone, st);
    case 1: return launch_group_cfg<32, 128, 1, 4, KS, TW, 1, RAG, LIMB>(jobs, n, alone, st);
    case 2: return launch_group_cfg<64, 64, 2, 2, KS, TW, 1, RAG, LIMB>(jobs, n, alone, st);
    case 3: return launch_group_cfg<64, 128, 2, 2, KS, TW, 1, RAG, LIMB>(jobs, n, alone, st);
    case 4: return launch_group_cfg<128, 64, 2, 2, KS, TW, 1, RAG, LIMB>(jobs, n, alone, st);
    default: return launch_group_cfg<128, 128, 2, 2, KS, TW, 1, RAG, LIMB>(jobs, n, alone, st);
  }
}

template <int KS, int TW>
static int launch_group_tw(int rag, int code, WgradTiledArgs* jobs, int n, bool alone, hipStream_t st) {
  const bool limb = wg_use_limbs(KS, TW, code, rag);
  switch (rag * 2 + limb) {
    case 0: return launch_group_code<KS, TW, 0, 0>(code, jobs, n, alone, st);
    case 1: return launch_group_code<KS, TW, 0, 1>(code, jobs, n, alone, st);
    case 2: return launch_group_code<KS, TW, 1, 0>(code, jobs, n, alone, st);
    case 3: return launch_group_code<KS, TW, 1, 1>(code, jobs, n, alone, st);
    case 4: return launch_group_code<KS, TW, 2, 0>(code, jobs, n, alone, st);
    default: return launch_group_code<KS, TW, 2, 1>(code, jobs, n, alone, st);
  }
}

// the one dispatcher over (kernel size, tile width, RAG); the tile widths are those of tiled_tw / tiled_tw_ragged
static int launch_group(int ks, int tw, int rag, int code, WgradTiledArgs* jobs, int n, bool alone, hipStream_t st) {
  if (ks == 1 && tw == 32) return launch_group_tw<1, 32>(rag, code, jobs, n, alone, st);
  if (ks == 1 && tw == 16) return launch_group_tw<1, 16>(rag, code, jobs, n, alone, st);
  if (ks == 1 && tw == 8) return launch_group_tw<1, 8>(rag, code, jobs, n, alone, st);
  if (ks == 3 && tw == 16) return launch_group_tw<3, 16>(rag, code, jobs, n, alone, st);
  if (ks == 3 && tw == 8) return launch_group_tw<3, 8>(rag, code, jobs, n, alone, st);
  return RSIS_ERR_ARG;
}

static WgradTiledArgs tiled_args(const WgradArgs& w) {
  WgradTiledArgs a = {};
  a.dy = w.dy; a.x = w.x; a.dw = w.dw; a.B = w.B; a.Cs = w.Cs; a.H = w.H; a.W = w.W; a.Cout = w.Cout;
  a.ldo = w.ldo; a.n_off = w.n_off; a.interleave_hid = w.interleave_hid;
  return a;
}

// n weight gradients that rsis_wgrad_tiled_supported accepts, all with the same kernel size: bucketed by (tile width, tile
// configuration), one grouped launch per bucket (per RSIS_WG_MAXJ jobs of a bucket)
static int tiled_launch_jobs(const WgradArgs* w, int n, int ks, bool alone, hipStream_t st) {
  if (n < 1) return RSIS_OK;
  WgradTiledArgs* all = (WgradTiledArgs*)malloc(sizeof(WgradTiledArgs) * n * 2);
  int* key = (int*)malloc(sizeof(int) * n);
  if (!all || !key) { free(all); free(key); return RSIS_ERR_LAUNCH; }
  WgradTiledArgs* bucket = all + n;
  for (int j = 0; j < n; ++j) {
    WgradTiledArgs& a = all[j] = tiled_args(w[j]);
    const int twa = tiled_tw(a.H, a.W, ks);
    if (twa) key[j] = twa * 8 + tiled_cfg_code(a, ks, twa, !alone);
    else {                      // ragged map: 1024 = dword DMA (RAG 1), 2048 = whole dwordx4 groups (RAG 2)
      if (ks == 1 && (a.H * a.W) % 4 == 0) { a.W = a.H * a.W; a.H = 1; }      // a 1x1 walks the flattened map
      key[j] = (a.W % 4 == 0 ? 2048 : 1024) + tiled_tw_ragged(a.W, ks) * 8 + tiled_cfg_code_single(a, ks);
    }
  }
  int rc = RSIS_OK;
  for (int j = 0; j < n && rc == RSIS_OK; ++j) {
    if (key[j] < 0) continue;
    const int k = key[j];
    int m = 0;
    for (int i = j; i < n; ++i)
      if (key[i] == k) { bucket[m++] = all[i]; key[i] = -1; }
    rc = launch_group(ks, (k & 1023) / 8, k >> 10, k % 8, bucket, m, alone, st);
  }
  free(all); free(key);
  return rc;
}

int rsis_launch_conv_wgrad_tiled_group(const WgradArgs* w, int n, int ks, hipStream_t st) { return tiled_launch_jobs(w, n, ks, false, st); }
// one weight gradient in a launch of its own: a group of one job under the split plan of a single launch
int rsis_launch_conv_wgrad_tiled(const WgradArgs& w, int ks, hipStream_t st) { return tiled_launch_jobs(&w, 1, ks, true, st); }

// true when the LDS-DMA tiled kernel covers this weight gradient (stride 1, "same" padding, tile-aligned map, 32-bit offsets)
bool rsis_wgrad_tiled_supported(const WgradArgs& w, int ks) {
  if (!(ks == 1 || ks == 3) || w.stride != 1 || w.pad != ks / 2 || w.H != w.Ho || w.W != w.Wo) return false;
  static const bool ragged_on = !(getenv("RSIS_WGRAD_RAGGED") && getenv("RSIS_WGRAD_RAGGED")[0] == '0');
  if (tiled_tw(w.H, w.W, ks) == 0 && !ragged_on) return false;      // (ragged maps: the RAG instantiations, grouped launch)
  const long img = (long)w.H * w.W * 4;
  return (long)w.Cout * img < (1L << 30) && (long)w.Cs * img < (1L << 30);
}
