// Dropout of the recurrent decoder (reference model.py:137-182: Dropout2d on every level's hidden state, Dropout on the class / stop
// head features) as SCALES the decoder's kernels fold in: one counter-based generator launch per sequence fills them, two small
// element-wise kernels apply the head masks.  The rule every word below follows is stated in include/rsis_hip.h (rsis_dropout_scales)
// and restated in numpy by rsis_amd/dropout.py.
#include "launchers.h"

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct DropScaleArgs {
  float* out[3];
  float p[3];
  long n;                  // elements per array
};

// thread = one Philox block = 4 consecutive elements of one array.  Every block reads the state before it takes a ticket; the block that
// takes the last ticket knows that all have read, advances the call counter and hands the ticket word back at zero.
__global__ __launch_bounds__(256) void dropout_scales_kernel(unsigned* __restrict__ state, const DropScaleArgs a) {
  __shared__ unsigned st[4];
  if (threadIdx.x == 0) {
    st[0] = state[0]; st[1] = state[1]; st[2] = state[2]; st[3] = state[3];
    __threadfence();
    const unsigned ticket = atomicAdd(state + 4, 1u);
    if (ticket == gridDim.x - 1) {
      const unsigned long long c = (((unsigned long long)st[3] << 32) | st[2]) + 1ull;
      state[2] = (unsigned)c;
      state[3] = (unsigned)(c >> 32);
      state[4] = 0u;
    }
  }
  __syncthreads();
  const unsigned k0 = st[0], k1 = st[1], call_lo = st[2], call_hi = st[3];
  const long n4 = (a.n + 3) >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < 3 * n4; q += (long)gridDim.x * 256) {
    const int arr = (int)(q / n4);
    const long j = q - arr * n4;
    unsigned w[4];
    philox4x32_10((unsigned)j, (unsigned)arr, call_lo, call_hi, k0, k1, w);
    const float p = a.p[arr];
    const float keep = 1.0f / (1.0f - p);
    float* o = a.out[arr];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long e = j * 4 + k;
      const float u = (float)(w[k] >> 8) * 5.9604644775390625e-8f;       // 2^-24: u in [0, 1), exact
      if (e < a.n) o[e] = u >= p ? keep : 0.f;
    }
  }
}

int rsis_l_dropout_scales(unsigned* state, float* s2, float* mc, float* ms, long n, float p2, float pc, float ps, hipStream_t st) {
  DropScaleArgs a;
  a.out[0] = s2; a.out[1] = mc; a.out[2] = ms;
  a.p[0] = p2; a.p[1] = pc; a.p[2] = ps;
  a.n = n;
  const long threads = 3 * ((n + 3) >> 2);
  long grid = (threads + 255) / 256;
  if (grid > 256) grid = 256;
  hipLaunchKernelGGL(dropout_scales_kernel, dim3((unsigned)grid), dim3(256), 0, st, state, a);
  return rsis_check_launch();
}

// side <- s2 * side (the Dropout2d scale of a plane commutes with its max-pool), side_c = mc * side, side_s = ms * side
__global__ __launch_bounds__(256) void dropout_heads_mask_kernel(float* __restrict__ side, const float* __restrict__ s2, const float* __restrict__ mc,
                                                                 const float* __restrict__ ms, float* __restrict__ side_c, float* __restrict__ side_s,
                                                                 long n) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float v = s2[e] * side[e];
  side[e] = v;
  side_c[e] = mc[e] * v;
  side_s[e] = ms[e] * v;
}
// dside = mc * d(side_c) + ms * d(side_s)  (a null gradient is zero)
__global__ __launch_bounds__(256) void dropout_heads_mask_bwd_kernel(const float* __restrict__ dc, const float* __restrict__ ds, const float* __restrict__ mc,
                                                                     const float* __restrict__ ms, float* __restrict__ dside, long n) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float a = dc ? mc[e] * dc[e] : 0.f;
  const float b = ds ? ms[e] * ds[e] : 0.f;
  dside[e] = a + b;
}

int rsis_l_dropout_heads_mask(float* side, const float* s2, const float* mc, const float* ms, float* side_c, float* side_s, long n, hipStream_t st) {
  if ((n + 255) / 256 > 0x7FFFFFFFL) return RSIS_ERR_ARG;
  hipLaunchKernelGGL(dropout_heads_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, side, s2, mc, ms, side_c, side_s, n);
  return rsis_check_launch();
}
int rsis_l_dropout_heads_mask_bwd(const float* dc, const float* ds, const float* mc, const float* ms, float* dside, long n, hipStream_t st) {
  if ((n + 255) / 256 > 0x7FFFFFFFL) return RSIS_ERR_ARG;
  hipLaunchKernelGGL(dropout_heads_mask_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dc, ds, mc, ms, dside, n);
  return rsis_check_launch();
}
