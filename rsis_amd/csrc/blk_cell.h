// The channel-blocked bf16 cell ("blk") and the pieces the kernels on it share, one copy each.  Device code: included by
// conv_blk.hip, conv_blk_dec.hip, blk_dec.hip, blk_norm.hip, upconv_out.hip, conv_bf16.hip, pack.hip and wgrad_parts.h.
//
// THE CONTRACT.  A logical [B][C][H][W] tensor is stored as bf16 [B][C/8][H][W][8]: one 16-byte CELL holds channels 8 cb .. 8 cb + 7
// of one pixel, channel 8 cb + 2 k in the low half of dword k and channel 8 cb + 2 k + 1 in its high half.  Every kernel computes in
// fp32 on the exact values of its bf16 inputs and rounds ONCE, to nearest even, at each blk store: blk_pack2 is that rounding and
// the only one, blk_lo / blk_hi are the exact way back.
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void* lds_vp_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

#define RSIS_OOB 0x7FFFFFF0u       // a byte offset outside every buffer descriptor: the load returns 0, the store is dropped
#define RSIS_VMCNT(N) __builtin_amdgcn_s_waitcnt(0x0F70 | ((N) & 15) | (((N) >> 4) << 14))
#ifndef XCD_CHUNKED
#define XCD_CHUNKED 1
#endif

// ---- the cell ----
__device__ __forceinline__ unsigned blk_pack2(float lo, float hi) {      // two fp32 -> one dword of two bf16 (v_cvt_pk_bf16_f32)
  const f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}
__device__ __forceinline__ float blk_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float blk_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
__device__ __forceinline__ u32x4 blk_cell_pack(const float (&v)[8]) {
  u32x4 c;
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = blk_pack2(v[2 * k], v[2 * k + 1]);
  return c;
}
__device__ __forceinline__ void blk_cell_unpack(const u32x4 c, float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[2 * k] = blk_lo(c[k]); v[2 * k + 1] = blk_hi(c[k]); }
}

// ---- BatchNorm on blk tensors: y = relu?(x * sc + sh (+ res)) with sc = gamma * rstd, sh = beta - mean * sc, in this order: the
//      scale, then the residual, then the ReLU.  The ONE statement of the arithmetic: the apply kernels of blk_norm.hip, the mask
//      recomputation of their backward and the folded epilogue of conv_blk_kernel give the same bits because they call these.
//      (Not the fp32 path's rsis_bn_affine / rsis_bn_apply of common.h: 1 / sqrtf and explicit fmaf there, rsqrtf and contracted
//      expressions here.) ----
__device__ __forceinline__ float blk_bn_rstd(float var, float eps) { return rsqrtf(var + eps); }
__device__ __forceinline__ void blk_bn_affine(float gamma, float beta, float mean, float rstd, float& sc, float& sh) {
  sc = gamma * rstd;
  sh = beta - mean * sc;
}
// the scale; callers then add the residual, then apply the ReLU (a helper around all three changed the instructions of the apply kernels)
__device__ __forceinline__ float blk_bn_apply(float x, float sc, float sh) { return x * sc + sh; }

// ---- the block program of the MFMA convolutions on cells (conv_blk_kernel, bd_body of conv_blk_dec.hip, and conv_bf16.hip, which
//      builds the same cells in LDS from fp32): 256 threads = WGM x WGN waves, a wave owns 32 output channels x TN groups of 32
//      pixels.  (The helpers end where they do because hipcc compiles each kernel to the same instructions as with the text in
//      place: a helper around the whole tap loop nest, around woff or around the epilogue's pixel did not.) ----

// block -> co tile (co_t) and spatial tile (returned; >= n_px_tiles: no tile, the grid is n_co_tiles * 8 * cdiv(n_px_tiles, 8)).
// Blocks b, b + 8, ... share an XCD: a tile's co tiles stay on one L2.
// (XCD x owns the contiguous range [x * chunk, (x + 1) * chunk) of the spatial tiles: blocks b, b + 8, ... -- the ones this XCD
//  runs one after the other -- are NEIGHBOURING tiles, so the halo rows / columns two tiles share are L2 hits instead of a
//  second fetch from HBM by another XCD.  Measured against the round-robin map `(q / n_co_tiles) * 8 + xcd` (a build with
//  -DXCD_CHUNKED=0): the bf16 gate launch of the 112 x 112 level 48.4 -> 33.6 us, the fp32 128 x 128 level 83.7 -> 79.3 us.)
__device__ __forceinline__ int blk_tile_of_block(const int bid, const int n_co_tiles, const int n_px_tiles, int& co_t) {
  const int xcd = bid & 7, q = bid >> 3;
  co_t = q % n_co_tiles;
  return XCD_CHUNKED ? xcd * ((n_px_tiles + 7) >> 3) + q / n_co_tiles : (q / n_co_tiles) * 8 + xcd;
}
// spatial tile -> image b0 and the origin (x0, y0) of its TW x TH pixels; returns the tiles per image
template <int TW, int TH>
__device__ __forceinline__ int blk_tile_origin(const int sp_t, const int W, const int H, int& b0, int& x0, int& y0) {
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int tx = sp_t % tiles_x;
  const int ty = (sp_t / tiles_x) % tiles_y;
  b0 = sp_t / (tiles_x * tiles_y);
  x0 = tx * TW; y0 = ty * TH;
  return tiles_x * tiles_y;
}

// per-lane LDS read base (in cells; the rest are immediates in the unrolled loop) of the wave's j-th group of 32 pixels: the stage
// is [channel block][PH][PW] cells of activations (IMS = PH * PW); the half wave `hi` reads the odd channel blocks
template <int TN, int TW, int PW, int IMS>
__device__ __forceinline__ int blk_xoff(const int wn, const int j, const int l31, const int hi) {
  const int pp = (wn * TN + j) * 32 + l31;
  const int x = pp % TW, y = pp / TW;
  return hi * IMS + y * PW + x;
}

__device__ __forceinline__ f32x16 blk_acc_zero() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// One tap of a 16-channel step on a landed stage: one weight cell per lane, TN activation cells, TN MFMAs.  A chunk is this over
// (kk, r, s) at Xs = stage + 2 kk IMS + r PW + s and Wa = weight stage + woff + ((r KS + s) NCB + 2 kk) BM, woff = hi BM + wm 32 + l31
// (weights: [tap][channel block][BM] cells).
template <int TN>
__device__ __forceinline__ void blk_mfma_tap(const u32x4* Xs, const u32x4* Wa, const int (&xoff)[TN], f32x16 (&acc)[TN]) {
  const bf16x8 a = __builtin_bit_cast(bf16x8, *Wa);
  bf16x8 b[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) b[j] = __builtin_bit_cast(bf16x8, Xs[xoff[j]]);
#pragma unroll
  for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[j], acc[j], 0, 0, 0);
}

// Epilogue.  Accumulator column = pixel l31, rows 4 g + i (i = 0..3) of a lane = channels co_base + 8 g + 4 hi + i: the half cell
// [4 hi, 4 hi + 4) of channel block co_base / 8 + g, one 8-byte store at this byte offset inside an image's [Cb][HW] cells.
// (An addend of the output's shape is fetched at these offsets for the whole tile BEFORE the first store and outside any
//  per-element condition: with the load inside `if (has_add)` hipcc branches around each one and waits vmcnt(0) behind it -- 4 TN
//  dependent L2 round trips per wave, each also draining the stores issued so far.)
__device__ __forceinline__ unsigned blk_half_off(const int cb, const int HW, const int osp, const int hi) {
  return (unsigned)(cb * HW + osp) * 16u + 8u * hi;
}
