// Flat fused SGD (with momentum) and RMSprop steps: the other two rules of the reference's get_optimizer (utils/utils.py:78-87),
// torch.optim.SGD / torch.optim.RMSprop semantics incl. L2 weight decay, over a flat fp32 parameter range and its one state buffer.
// (The Adam step lives in pointwise.hip: adam_kernel.)  Both read p, g and the state and write p and the state: 20 B per parameter,
// HBM-bound.  The range may start at any parameter offset of the flat buffers: a scalar head up to 16-byte alignment, a float4 body,
// a scalar tail.
#include "common.h"
#include "launchers.h"

enum { RULE_SGD = 0, RULE_RMSPROP = 1 };

// d = g * gscale + wd * p (gscale: 1 / world after the SUM all-reduce, folded in as adam_kernel does), then
//   SGD     (c0 = momentum):         s = mu * s + d;                          p -= lr * s
//           (dampening 0, no Nesterov; a zero buffer makes the first step s = d, torch's buf = d.clone())
//   RMSprop (c0 = alpha, c1 = eps):  s = alpha * s + (1 - alpha) * d * d;     p -= lr * d / (sqrt(s) + eps)
//           (no momentum, not centred)
template <int RULE>
__device__ __forceinline__ void flat_rule_update(float& p, float g, float& s, float lr, float c0, float c1, float wd, float gscale) {
  const float d = g * gscale + wd * p;
  if (RULE == RULE_SGD) {
    s = c0 * s + d;
    p -= lr * s;
  } else {
    s = c0 * s + (1.f - c0) * (d * d);
    p -= lr * (d / (sqrtf(s) + c1));
  }
}

// elements [head, head + 4 nv) as float4 (p, g and s all 16-byte aligned there), the fewer than 4 before and after them one by one;
// head = n (nv = 0) when the three pointers are not aligned alike
template <int RULE>
__global__ __launch_bounds__(256) void flat_rule_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s,
                                                        long n, long head, long nv, float lr, float c0, float c1, float wd,
                                                        float gscale) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p + head);
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g + head);
  f32x4* __restrict__ s4 = reinterpret_cast<f32x4*>(s + head);
  for (long i = tid; i < nv; i += stride) {
    f32x4 pv = p4[i], sv = s4[i];
    const f32x4 gv = g4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = pv[k], sk = sv[k];
      flat_rule_update<RULE>(pk, gv[k], sk, lr, c0, c1, wd, gscale);
      pv[k] = pk;
      sv[k] = sk;
    }
    p4[i] = pv;
    s4[i] = sv;
  }
  const long tail = head + 4 * nv;
  const long ns = head + (n - tail);
  for (long i = tid; i < ns; i += stride) {
    const long e = i < head ? i : tail + (i - head);
    float pe = p[e], se = s[e];
    flat_rule_update<RULE>(pe, g[e], se, lr, c0, c1, wd, gscale);
    p[e] = pe;
    s[e] = se;
  }
}

// launcher (called from api.hip); n >= 1
int rsis_l_flat_rule(int rule, float* p, const float* g, float* s, long n, float lr, float c0, float c1, float wd, float gscale,
                     hipStream_t st) {
  const uintptr_t ap = (uintptr_t)p, ag = (uintptr_t)g, as = (uintptr_t)s;
  long head = n;
  if (((ap ^ ag) & 15) == 0 && ((ap ^ as) & 15) == 0 && (ap & 3) == 0) {
    head = (long)(((16 - (ap & 15)) & 15) >> 2);
    if (head > n) head = n;
  }
  const long nv = (n - head) / 4;
  const long ns = n - 4 * nv;
  const int grid = ew_grid(nv > ns ? nv : ns);
  if (rule == RULE_SGD)
    hipLaunchKernelGGL(flat_rule_kernel<RULE_SGD>, dim3(grid), dim3(256), 0, st, p, g, s, n, head, nv, lr, c0, c1, wd, gscale);
  else
    hipLaunchKernelGGL(flat_rule_kernel<RULE_RMSPROP>, dim3(grid), dim3(256), 0, st, p, g, s, n, head, nv, lr, c0, c1, wd, gscale);
  return rsis_check_launch();
}
