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
