// The limb flavour of the direct 3x3 / stride 1 / pad 1 conv: fp32 operands as three bf16 limbs each (limb_split.h), six products per
// K16 step on v_mfma_f32_32x32x16_bf16, fp32 accumulation -- 192 matrix cycles per 16 reduction values against 512 on
// v_mfma_f32_32x32x2_f32.  Training calls only (rsis_conv2d_fwd with tile + 100, rsis_conv2d_dgrad, rsis_convlstm_fwd with act_out) and
// only where the caller's routing asks for it (RSIS_DTYPE_F32_LIMB); everything else keeps the f32 body of conv3x3_direct.hip.
//
// This header is the STAGING and the MFMA LOOP of that flavour.  It fills the accumulators of conv3x3_direct_body (same 32 x 32 tile
// layout as the f32 MFMA: column = pixel l31, rows (r & 3) + 8 (r >> 2) + 4 hi), which then runs the ONE epilogue both flavours share.
//   * Activations: fp32 NCHW patches with halo (zero-filled by the descriptor's range check, as the channel tail), eight channels of a
//     pixel per task through registers, split ONCE by rsis_limb_pack8_cells into three 16-byte cells:  Xs[limb][c8 block][PH][PW].
//   * Weights: pre-split by pack.hip (PACK_LIMB_FWD / PACK_LIMB_DGRAD), per 16-channel chunk 3 limbs x 9 taps x 2 blocks = 54 cell rows
//     of ldw cells:  row ((q * 3 + limb) * 9 + tap) * 2 + cb.  The block copies its BM columns of the 54 rows:  Ws[limb][tap][cb][BM].
//   * One LDS stage, two chunks in flight: the loads of chunk t + 1 (activations AND weights) are issued into registers before the
//     MFMAs of chunk t and written to LDS between two barriers after them.  A second LDS stage would take the 32-row block from 45 / 60 KB
//     to 90 / 120 KB, one block per CU; the registers (16-24 for the patch, 28 for the weights) are there.
//   * Chunks are 16 channels x 9 taps = 9 K16 steps, never straddling a source (sources are multiples of 8: a 24-channel source has a
//     half-empty second chunk).  Per tap a wave reads 3 weight cells and 3 TN patch cells for 6 TN MFMAs, B limb 2 first (RSIS_LIMB_PB).
#pragma once
#include "blk_cell.h"
#include "limb_split.h"

#define RSIS_CKL 16          // input channels per chunk of the limb flavour (one K16 step per tap)
#define RSIS_LIMB_ROWS 54    // packed cell rows per chunk: 3 limbs x 9 taps x 2 channel blocks

// floats of LDS one block needs (one stage of patch + weight cells, three limbs each)
template <int BM, int TW, int TH>
constexpr int limb_lds_floats() {
  return 3 * (2 * (TW + 2) * (TH + 2) + 9 * 2 * BM) * 4;
}

template <int BM, int TW, int TH, int TN>
__device__ __forceinline__ void rsis_limb_mainloop(const ConvArgs& p, const int b0, const int x0, const int y0, const int co_t, const int wm, const int wn,
                                                   float* const lds, f32x16 (&acc)[TN]) {
#if __HIP_DEVICE_COMPILE__
  typedef const float __attribute__((address_space(1)))* gcf_t;
  constexpr int NCB = RSIS_CKL / 8;
  constexpr int PW = TW + 2, PH = TH + 2, IMS = PH * PW;
  constexpr int XC1 = NCB * IMS, XC = 3 * XC1;              // patch cells per limb / per stage
  constexpr int WC1 = 9 * NCB * BM, WC = 3 * WC1;           // weight cells per limb / per stage
  constexpr int NXT = (XC1 + 255) / 256, NWT = (WC + 255) / 256;
  static_assert(4 * (XC + WC) == limb_lds_floats<BM, TW, TH>(), "LDS size helper out of sync");
  u32x4* const Xs = reinterpret_cast<u32x4*>(lds);
  u32x4* const Ws = Xs + XC;

  const gcf_t src0 = (gcf_t)p.src[0], src1 = (gcf_t)p.src[1], src2 = (gcf_t)p.src[2];
  const int C0 = p.C[0], C1 = p.C[1], C2 = p.C[2];
  const int q0 = (C0 + RSIS_CKL - 1) / RSIS_CKL, q1 = (C1 + RSIS_CKL - 1) / RSIS_CKL, q2 = (C2 + RSIS_CKL - 1) / RSIS_CKL;
  const int nq = q0 + q1 + q2;
  const int H = p.H, W = p.W, HW = H * W, ldw = p.ldw;
  const int tid = threadIdx.x;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;

  unsigned xvo[NXT];
#pragma unroll
  for (int i = 0; i < NXT; ++i) {
    const int e = tid + i * 256;
    const int cb = e / IMS, rem = e - cb * IMS;
    const int py = rem / PW, pxx = rem - py * PW;
    const int gy = y0 + py - 1, gx = x0 + pxx - 1;
    const bool ok = (e < XC1) && ((unsigned)gy < (unsigned)H) && ((unsigned)gx < (unsigned)W);
    xvo[i] = ok ? (unsigned)(cb * 8 * HW + gy * W + gx) * 4u : RSIS_OOB;
  }
  unsigned wvo[NWT];
#pragma unroll
  for (int i = 0; i < NWT; ++i) {
    const int idx = tid + i * 256;
    wvo[i] = idx < WC ? (unsigned)((idx / BM) * ldw + idx % BM) * 16u : RSIS_OOB;
  }
  const unsigned chs = (unsigned)HW * 4u;

  int xoff[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) xoff[j] = blk_xoff<TN, TW, PW, IMS>(wn, j, l31, hi);
  const int woff = hi * BM + wm * 32 + l31;
  const char* const wbase = (const char*)p.wp + (size_t)co_t * BM * 16;

  int cs = 0, cq = 0;      // source index, chunk index inside the source
  if (q0 == 0) { cs = 1; if (q1 == 0) cs = 2; }
  float rx[NXT][8];
  u32x4 rw[NWT];
  // all loads of chunk QG into registers: 8 channels per patch task, one cell per weight task
#define LIMB_ISSUE(QG)                                                                                             \
  {                                                                                                                \
    gcf_t src = src0; int Cs = C0;                                                                                 \
    if (cs == 1) { src = src1; Cs = C1; }                                                                          \
    if (cs == 2) { src = src2; Cs = C2; }                                                                          \
    const int c0 = cq * RSIS_CKL;                                                                                  \
    const int cn = min(RSIS_CKL, Cs - c0);                                                                         \
    const float* xb = (const float*)src + ((size_t)b0 * Cs + c0) * HW;                                             \
    const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, cn * HW * 4, 0x00020000);   \
    _Pragma("unroll") for (int i = 0; i < NXT; ++i)                                                                \
      _Pragma("unroll") for (int c = 0; c < 8; ++c)                                                                \
        rx[i][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx_, xvo[i] + c * chs, 0, 0));   \
    const char* wrow = wbase + (size_t)(QG) * RSIS_LIMB_ROWS * ldw * 16;                                           \
    const __amdgpu_buffer_rsrc_t rw_ = __builtin_amdgcn_make_buffer_rsrc((void*)wrow, 0, RSIS_LIMB_ROWS * ldw * 16, 0x00020000); \
    _Pragma("unroll") for (int i = 0; i < NWT; ++i) rw[i] = __builtin_amdgcn_raw_buffer_load_b128(rw_, wvo[i], 0, 0); \
    if (++cq == (cs == 0 ? q0 : (cs == 1 ? q1 : q2))) { cq = 0; ++cs; if (cs == 1 && q1 == 0) ++cs; }             \
  }
  // registers -> LDS: the patch values are split here, once per staged element
#define LIMB_STORE()                                                                                               \
  {                                                                                                                \
    _Pragma("unroll") for (int i = 0; i < NXT; ++i) {                                                              \
      const int e = tid + i * 256;                                                                                 \
      if (XC1 % 256 == 0 || e < XC1) {                                                                             \
        unsigned c0_[4], c1_[4], c2_[4];                                                                           \
        rsis_limb_pack8_cells(rx[i], c0_, c1_, c2_);                                                               \
        const u32x4 v0 = {c0_[0], c0_[1], c0_[2], c0_[3]}, v1 = {c1_[0], c1_[1], c1_[2], c1_[3]}, v2 = {c2_[0], c2_[1], c2_[2], c2_[3]}; \
        Xs[e] = v0; Xs[XC1 + e] = v1; Xs[2 * XC1 + e] = v2;                                                        \
      }                                                                                                            \
    }                                                                                                              \
    _Pragma("unroll") for (int i = 0; i < NWT; ++i) {                                                              \
      const int idx = tid + i * 256;                                                                               \
      if (WC % 256 == 0 || idx < WC) Ws[idx] = rw[i];                                                              \
    }                                                                                                              \
  }
  if (nq > 0) {
    LIMB_ISSUE(0)
    LIMB_STORE()
  }
  __syncthreads();
  for (int t = 0; t < nq; ++t) {
    const bool more = t + 1 < nq;
    if (more) LIMB_ISSUE(t + 1)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const u32x4* Xt = Xs + r * PW + s;
        const u32x4* Wt = Ws + woff + ((r * 3 + s) * NCB) * BM;
        bf16x8 a[3], b[3][TN];
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          a[l] = __builtin_bit_cast(bf16x8, Wt[l * WC1]);
#pragma unroll
          for (int j = 0; j < TN; ++j) b[l][j] = __builtin_bit_cast(bf16x8, Xt[l * XC1 + xoff[j]]);
        }
#pragma unroll
        for (int q = 0; q < RSIS_LIMB_PRODUCTS; ++q)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[RSIS_LIMB_PA(q)], b[RSIS_LIMB_PB(q)][j], acc[j], 0, 0, 0);
      }
    __syncthreads();            // every wave has read the stage (after the last chunk: the stage is dead, the epilogue may park in it)
    if (more) {
      LIMB_STORE()
      __syncthreads();
    }
  }
#undef LIMB_ISSUE
#undef LIMB_STORE
#endif
}
