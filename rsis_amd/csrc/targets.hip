// Data-layer targets of a whole batch on the device (reference src/dataloader/dataset.py:86-146 sequence_from_masks followed by
// utils.batch_to_var): what dataloader/targets.py builds with a Python loop over the images (per image a torch.unique host sync, a
// sort, a k x HW comparison and a masked min), as three launches and one host sync per BATCH:
//   init      : counts[B][256] = 0, minclass[B][256] = INT_MAX, flag = 0
//   histogram : per image the area of every id and the smallest class under it; LDS atomics per block, then one global integer atomic
//               per (block, id present); an id outside 0..255 raises the flag (the host reads it: RSIS_ERR_UNSUPPORTED, nothing written)
//   write     : every block ranks the <= 256 ids of its image from the histogram (area descending, equal areas: larger id first, the
//               smallest id present dropped) into an id -> row table in LDS and writes its pixels of all T rows of y_mask; block 0 of an
//               image also writes y_class / sw_mask / sw_class.
// Integer counts only, so the result is the same whatever the order of the atomics.  Bound: HBM, the B * T * HW * 4 bytes of y_mask.
#include "common.h"
#include "launchers.h"
#include <limits.h>

#define TGT_IDS 256

__global__ __launch_bounds__(256) void targets_init_kernel(int* __restrict__ work, long n_cnt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_cnt) work[i] = 0;                           // counts
  else if (i < 2 * n_cnt) work[i] = INT_MAX;            // minclass
  else if (i == 2 * n_cnt) work[i] = 0;                 // flag
}

__global__ __launch_bounds__(256) void targets_hist_kernel(const int* __restrict__ ins, const int* __restrict__ seg, int HW,
                                                           int* __restrict__ counts, int* __restrict__ mincls, int* __restrict__ flag) {
  __shared__ int cnt[TGT_IDS], mn[TGT_IDS];
  const int b = blockIdx.y, tid = threadIdx.x;
  cnt[tid] = 0;
  mn[tid] = INT_MAX;
  __syncthreads();
  const int* ib = ins + (size_t)b * HW;
  const int* sb = seg + (size_t)b * HW;
  bool bad = false;
  for (long e = (long)blockIdx.x * 256 + tid; e < HW; e += (long)gridDim.x * 256) {
    const int id = ib[e];
    if ((unsigned)id >= TGT_IDS) { bad = true; continue; }
    atomicAdd(&cnt[id], 1);
    atomicMin(&mn[id], sb[e]);
  }
  if (bad) atomicOr(flag, 1);
  __syncthreads();
  if (cnt[tid]) {
    atomicAdd(&counts[(size_t)b * TGT_IDS + tid], cnt[tid]);
    atomicMin(&mincls[(size_t)b * TGT_IDS + tid], mn[tid]);
  }
}

__global__ __launch_bounds__(256) void targets_write_kernel(const int* __restrict__ ins, int HW, int T, const int* __restrict__ counts,
                                                            const int* __restrict__ mincls, float* __restrict__ y_mask,
                                                            long long* __restrict__ y_class, float* __restrict__ sw_mask,
                                                            float* __restrict__ sw_class) {
  __shared__ int cnt[TGT_IDS], row[TGT_IDS];
  __shared__ int bg, n_inst;
  const int b = blockIdx.y, tid = threadIdx.x;
  cnt[tid] = counts[(size_t)b * TGT_IDS + tid];
  if (tid == 0) { bg = TGT_IDS; n_inst = 0; }
  __syncthreads();
  if (cnt[tid]) { atomicMin(&bg, tid); atomicAdd(&n_inst, 1); }
  __syncthreads();
  // row of id `tid`: the number of instances that come before it (larger area, or the same area and a larger id); -1 = not a row
  int r = -1;
  const int c = cnt[tid];
  if (c && tid != bg) {
    r = 0;
    for (int j = 0; j < TGT_IDS; ++j) {
      const int cj = cnt[j];
      if (j != bg && cj && (cj > c || (cj == c && j > tid))) ++r;
    }
    if (r >= T) r = -1;
  }
  row[tid] = r;
  const int n = n_inst - 1;                           // instances of the image (an image always has a background id: HW >= 1)
  if (blockIdx.x == 0) {
    // rows of instances through their own thread, the empty rows through a strided loop
    if (r >= 0) {
      y_class[(size_t)b * T + r] = (long long)mincls[(size_t)b * TGT_IDS + tid];
      sw_mask[(size_t)b * T + r] = 1.f;
      sw_class[(size_t)b * T + r] = 1.f;
    }
    for (int t = n + tid; t < T; t += 256) {
      y_class[(size_t)b * T + t] = 0;
      sw_mask[(size_t)b * T + t] = 0.f;
      sw_class[(size_t)b * T + t] = t == n ? 1.f : 0.f;
    }
  }
  __syncthreads();
  const int* ib = ins + (size_t)b * HW;
  float* yb = y_mask + (size_t)b * T * HW;
  for (long e = (long)blockIdx.x * 256 + tid; e < HW; e += (long)gridDim.x * 256) {
    const int rr = row[ib[e]];                         // ids were checked by the histogram pass: 0..255
    for (int t = 0; t < T; ++t) yb[(size_t)t * HW + e] = t == rr ? 1.f : 0.f;
  }
}

long rsis_l_targets_work_ints(int B) { return 2L * B * TGT_IDS + 1; }

int rsis_l_targets_from_maps(const int* ins, const int* seg, int B, int H, int W, int T, float* y_mask, long long* y_class, float* sw_mask,
                             float* sw_class, int* work, hipStream_t st) {
  const int HW = H * W;
  const long n_cnt = (long)B * TGT_IDS;
  int* counts = work;
  int* mincls = work + n_cnt;
  int* flag = work + 2 * n_cnt;
  hipLaunchKernelGGL(targets_init_kernel, dim3((unsigned)((2 * n_cnt + 1 + 255) / 256)), dim3(256), 0, st, work, n_cnt);
  long gx = ((long)HW + 256 * 16 - 1) / (256 * 16);   // 16 pixels per thread: few global atomics per id
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(targets_hist_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, st, ins, seg, HW, counts, mincls, flag);
  if (rsis_check_launch() != RSIS_OK) return RSIS_ERR_LAUNCH;
  int host_flag = 0;
  if (hipMemcpyAsync(&host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return RSIS_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return RSIS_ERR_LAUNCH;
  if (host_flag) return RSIS_ERR_UNSUPPORTED;
  long gw = ((long)HW + 256 * 4 - 1) / (256 * 4);
  if (gw > 4096) gw = 4096;
  hipLaunchKernelGGL(targets_write_kernel, dim3((unsigned)gw, (unsigned)B), dim3(256), 0, st, ins, HW, T, counts, mincls, y_mask, y_class,
                     sw_mask, sw_class);
  return rsis_check_launch();
}
