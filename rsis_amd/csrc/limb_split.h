// An fp32 value as the exact sum of three bf16 limbs, by truncation (conv_wgrad_tiled.hip: fp32 weight gradients on
// v_mfma_f32_32x32x16_bf16).
//     l0 = v with its low 16 bits cleared        r1 = v  - l0   (exact: r1 is the cleared bits, <= 16 significant bits)
//     l1 = r1 with its low 16 bits cleared       r2 = r1 - l1   (exact: <= 8 significant bits are left)
//     l2 = r2                                                    (its high half IS the value)
// so l0 + l1 + l2 == v bit for bit for every finite fp32 v, each limb has zero low 16 bits (its high half is its bf16 encoding),
// every limb has the sign of v or is zero, and nothing can overflow near FLT_MAX (|l0| <= |v|; rounding to nearest could carry
// into the exponent there).  Non-finite inputs give non-finite limbs, not necessarily of the same kind (inf - inf = NaN in r1):
// a product that uses them is non-finite as it is on the f32 MFMA, but an inf may turn into a NaN.
// Below |v| = 2^-103 the last residual can be a subnormal: the sum is still exact, but that limb keeps low bits which the kernel's
// pack (high halves only) drops -- less than 2^-126 in absolute terms.
// Plain C++ on purpose: tests/test_wgrad_limbs_split.py compiles this header with the host compiler.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSIS_LIMB_HD __host__ __device__
#else
#define RSIS_LIMB_HD
#endif

RSIS_LIMB_HD inline float rsis_limb_hi16(const float v) {      // v with the low 16 bits of its encoding cleared
  unsigned u;
  __builtin_memcpy(&u, &v, 4);
  u &= 0xFFFF0000u;
  float r;
  __builtin_memcpy(&r, &u, 4);
  return r;
}

RSIS_LIMB_HD inline void rsis_limb_split3(const float v, float& l0, float& l1, float& l2) {
  l0 = rsis_limb_hi16(v);
  const float r1 = v - l0;
  l1 = rsis_limb_hi16(r1);
  l2 = r1 - l1;
}

// two fp32 encodings -> one dword of two bf16 values by truncation: the high half of `even` in the low half, of `odd` in the high half
RSIS_LIMB_HD inline unsigned rsis_limb_pair(const float even, const float odd) {
  unsigned e, o;
  __builtin_memcpy(&e, &even, 4);
  __builtin_memcpy(&o, &odd, 4);
  return (e >> 16) | (o & 0xFFFF0000u);
}

// Eight consecutive fp32 values -> three 16-byte cells (the staged limb kernels of conv_wgrad_bf16.hip: split ONCE per staged element).
// Cell l holds limb l of all eight values, high halves only, element 2m in the low half of dword m and element 2m + 1 in its high
// half: a cell is one lane's bf16x8 MFMA fragment, as wg_limb_pack8 (conv_wgrad_tiled.hip) builds it in registers.
RSIS_LIMB_HD inline void rsis_limb_pack8_cells(const float (&v)[8], unsigned (&c0)[4], unsigned (&c1)[4], unsigned (&c2)[4]) {
  for (int m = 0; m < 4; ++m) {
    float lo[3], hi[3];
    rsis_limb_split3(v[2 * m], lo[0], lo[1], lo[2]);
    rsis_limb_split3(v[2 * m + 1], hi[0], hi[1], hi[2]);
    c0[m] = rsis_limb_pair(v[2 * m], v[2 * m + 1]);      // (limb 0 is the high half of v itself)
    c1[m] = rsis_limb_pair(lo[1], hi[1]);
    c2[m] = rsis_limb_pair(lo[2], hi[2]);
  }
}

// limb pairs (A limb, B limb) of one K16 step, smallest weight first: the six products with i + j <= 2 (weight >= 2^-16), the same six
// as wg_limb_pa / wg_limb_pb of conv_wgrad_tiled.hip.  Among the three of weight 2^-16 and the two of weight 2^-8 the order is
// (0,2) (2,0) (1,1) | (0,1) (1,0) | (0,0): B limb 2 is used first and then dead, B limb 1 lives over two adjacent products -- the 3x3
// kernel holds 12 registers of shifted windows per B limb, and with all three live to the end it spilled.
#define RSIS_LIMB_PRODUCTS 6
#define RSIS_LIMB_PA(q) ((q) == 1 ? 2 : ((q) == 2 || (q) == 4 ? 1 : 0))
#define RSIS_LIMB_PB(q) ((q) == 0 ? 2 : ((q) == 2 || (q) == 3 ? 1 : 0))
