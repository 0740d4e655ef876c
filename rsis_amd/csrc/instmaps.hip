// Class map and compact instance map of a batch of Cityscapes `*_instanceIds` images on the device (reference
// src/dataloader/cityscapes.py:67-92: np.unique over the id image, then one full-image compare per instance, on the host).
// An id is labelId * 1000 + k (24000..33999 for the evaluated classes), below 65536; the targets kernel (targets.hip) takes ids
// 0..255.  The compaction "rank among the distinct kept ids of the image" needs no sort: a 65536-bit presence bitmap per image and
// the prefix sum of its popcounts give the rank of any id.  Three launches, no host sync:
//   init     : work[B][2048] = 0
//   presence : every block ORs the kept ids of its pixels into a bitmap in LDS (8 KB, LDS atomicOr) and flushes the non-zero words
//              to work[b] with one global atomicOr each
//   map      : every block loads its image's 2048 words, scans their popcounts (exclusive prefix per word) and writes
//              seg = class, ins = 1 + prefix[id >> 5] + popcount(bits of the word below id) for its pixels
// Bitwise ORs and integer counts only: the result does not depend on the order of execution.  Bound: HBM (4 B read twice, 8 B
// written per pixel).
#include "common.h"
#include "launchers.h"

#define IM_WORDS 2048          // 65536 bits
#define IM_LABELS 66           // labels 0..65 (65535 / 1000)
#define IM_T 256

// class of a raw id under the table in LDS; 0 = not an instance.  A value outside 0..65535 counts as 0.
__device__ __forceinline__ int im_class(int raw, const int* tab, int n_labels) {
  if ((unsigned)raw > 65535u || raw < 1000) return 0;
  const int label = raw / 1000;
  return label < n_labels ? tab[label] : 0;
}

__global__ __launch_bounds__(IM_T) void instmaps_init_kernel(int* __restrict__ work, long n) {
  const long i = (long)blockIdx.x * IM_T + threadIdx.x;
  if (i < n) work[i] = 0;
}

__global__ __launch_bounds__(IM_T) void instmaps_presence_kernel(const int* __restrict__ raw, const int* __restrict__ class_of_label,
                                                                 int n_labels, int HW, unsigned int* __restrict__ work) {
  __shared__ unsigned int bm[IM_WORDS];
  __shared__ int tab[IM_LABELS];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < IM_WORDS; i += IM_T) bm[i] = 0u;
  if (tid < IM_LABELS) tab[tid] = tid < n_labels ? class_of_label[tid] : 0;
  __syncthreads();
  const int* rb = raw + (size_t)b * HW;
  int last = -1;                                      // (ids come in runs: one LDS atomic per change of value, not per pixel)
  for (long e = (long)blockIdx.x * IM_T + tid; e < HW; e += (long)gridDim.x * IM_T) {
    const int v = rb[e];
    if (v == last) continue;
    last = v;
    if (im_class(v, tab, n_labels) > 0) atomicOr(&bm[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
  unsigned int* wb = work + (size_t)b * IM_WORDS;
  for (int i = tid; i < IM_WORDS; i += IM_T) {
    const unsigned int w = bm[i];
    if (w) atomicOr(&wb[i], w);
  }
}

__global__ __launch_bounds__(IM_T) void instmaps_map_kernel(const int* __restrict__ raw, const int* __restrict__ class_of_label, int n_labels,
                                                            int HW, const unsigned int* __restrict__ work, int* __restrict__ ins,
                                                            int* __restrict__ seg) {
  __shared__ unsigned int bm[IM_WORDS];
  __shared__ int prefix[IM_WORDS];                    // kept ids of the image below word i
  __shared__ int tab[IM_LABELS];
  __shared__ int wsum[IM_T / 64];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned int* wb = work + (size_t)b * IM_WORDS;
  if (tid < IM_LABELS) tab[tid] = tid < n_labels ? class_of_label[tid] : 0;
  // thread t owns words 8t .. 8t+7
  unsigned int w[IM_WORDS / IM_T];
  int c = 0;
#pragma unroll
  for (int i = 0; i < IM_WORDS / IM_T; ++i) {
    w[i] = wb[tid * (IM_WORDS / IM_T) + i];
    bm[tid * (IM_WORDS / IM_T) + i] = w[i];
    c += __popc(w[i]);
  }
  int inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int run = inc - c;
#pragma unroll
  for (int i = 0; i < IM_T / 64; ++i)
    if (i < wv) run += wsum[i];
#pragma unroll
  for (int i = 0; i < IM_WORDS / IM_T; ++i) {
    prefix[tid * (IM_WORDS / IM_T) + i] = run;
    run += __popc(w[i]);
  }
  __syncthreads();
  const int* rb = raw + (size_t)b * HW;
  int* ib = ins + (size_t)b * HW;
  int* sb = seg + (size_t)b * HW;
  for (long e = (long)blockIdx.x * IM_T + tid; e < HW; e += (long)gridDim.x * IM_T) {
    const int v = rb[e];
    const int cls = im_class(v, tab, n_labels);
    int rank = 0;
    if (cls > 0) rank = 1 + prefix[v >> 5] + __popc(bm[v >> 5] & ((1u << (v & 31)) - 1u));
    ib[e] = rank;
    sb[e] = cls;
  }
}

long rsis_l_instance_maps_work_ints(int B) { return (long)B * IM_WORDS; }

int rsis_l_instance_maps(const int* raw, const int* class_of_label, int n_labels, int B, int H, int W, int* ins, int* seg, int* work,
                         hipStream_t st) {
  const int HW = H * W;
  const long n = (long)B * IM_WORDS;
  hipLaunchKernelGGL(instmaps_init_kernel, dim3((unsigned)((n + IM_T - 1) / IM_T)), dim3(IM_T), 0, st, work, n);
  long gp = ((long)HW + IM_T * 16 - 1) / (IM_T * 16);  // 16 pixels per thread: one flush of the bitmap per 4096 pixels
  if (gp > 1024) gp = 1024;
  hipLaunchKernelGGL(instmaps_presence_kernel, dim3((unsigned)gp, (unsigned)B), dim3(IM_T), 0, st, raw, class_of_label, n_labels, HW,
                     (unsigned int*)work);
  long gm = ((long)HW + IM_T * 8 - 1) / (IM_T * 8);    // 8 pixels per thread: the 8 KB bitmap load + scan per 2048 pixels
  if (gm > 4096) gm = 4096;
  hipLaunchKernelGGL(instmaps_map_kernel, dim3((unsigned)gm, (unsigned)B), dim3(IM_T), 0, st, raw, class_of_label, n_labels, HW,
                     (const unsigned int*)work, ins, seg);
  return rsis_check_launch();
}
