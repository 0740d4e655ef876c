// Offline preparation of Pascal VOC on the device (reference src/dataloader/pascal_precompute.py:36-101):
//   palette_to_ids_kernel : the colour PNGs -> id maps.  The reference does a Python dict lookup per pixel (dataset_utils.py
//                           convert_from_color_segmentation, marked "still too slow!!"); here the <= 256-entry (r, g, b, id) table sits in
//                           LDS as packed words and every thread compares its pixel against it.  First match wins, no match = 0.
//   idmap_rle_kernel      : the ground-truth records' run-length encoding.  One block per requested id walks the ROW-major id map in
//                           COLUMN-major element order (element e = x * h + y, pycocotools' order) and emits the run counts of the mask
//                           (idmap == id) -- the scheme of rle_encode_kernel (maskpost.hip): per chunk the threads count value changes, a
//                           block scan places their positions, a second pass turns positions into lengths -- without the k x hw byte masks.
#include "common.h"
#include "launchers.h"

__global__ __launch_bounds__(256) void palette_to_ids_kernel(const unsigned char* __restrict__ rgb, long npix,
                                                             const unsigned char* __restrict__ table, int ntab,
                                                             unsigned char* __restrict__ ids) {
  __shared__ unsigned int key[256];
  __shared__ unsigned char val[256];
  const int tid = threadIdx.x;
  if (tid < ntab) {
    key[tid] = (unsigned int)table[4 * tid] | ((unsigned int)table[4 * tid + 1] << 8) | ((unsigned int)table[4 * tid + 2] << 16);
    val[tid] = table[4 * tid + 3];
  }
  __syncthreads();
  for (long p = (long)blockIdx.x * 256 + tid; p < npix; p += (long)gridDim.x * 256) {
    const unsigned int c = (unsigned int)rgb[3 * p] | ((unsigned int)rgb[3 * p + 1] << 8) | ((unsigned int)rgb[3 * p + 2] << 16);
    unsigned char id = 0;
    for (int i = ntab - 1; i >= 0; --i)               // descending, so that the FIRST matching entry is the one kept
      if (key[i] == c) id = val[i];
    ids[p] = id;
  }
}

#define IRLE_T 1024   // threads per block
#define IRLE_E 16     // consecutive (column-major) elements per thread per chunk
__global__ __launch_bounds__(IRLE_T) void idmap_rle_kernel(const unsigned char* __restrict__ idmap, int h, int w,
                                                           const int* __restrict__ ids, unsigned int* __restrict__ counts, int cap,
                                                           int* __restrict__ nruns) {
  const int k = blockIdx.x;
  const int id = ids[k];
  const long len = (long)h * w;
  unsigned int* out = counts + (size_t)k * cap;
  __shared__ unsigned int wsum[IRLE_T / 64];
  __shared__ unsigned int running;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) running = 0;
  __syncthreads();
  // element e of the column-major mask: column e / h, row e % h of the row-major map
#define IRLE_AT(e) ((int)idmap[(size_t)((e) % h) * w + (size_t)((e) / h)] == id ? 1 : 0)
  for (long base = 0; base < len; base += (long)IRLE_T * IRLE_E) {
    const long j0 = base + (long)tid * IRLE_E;
    unsigned char v[IRLE_E + 1];
    v[0] = (j0 > 0 && j0 - 1 < len) ? IRLE_AT(j0 - 1) : 0;
#pragma unroll
    for (int i = 0; i < IRLE_E; ++i) {
      const bool ok = j0 + i < len;
      v[i + 1] = ok ? IRLE_AT(j0 + i) : v[i];
    }
    unsigned int c = 0;
#pragma unroll
    for (int i = 0; i < IRLE_E; ++i) c += (v[i + 1] != v[i]) ? 1u : 0u;
    unsigned int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned int woff = 0, total = 0;
#pragma unroll
    for (int i = 0; i < IRLE_T / 64; ++i) {
      const unsigned int s = wsum[i];
      if (i < wv) woff += s;
      total += s;
    }
    unsigned int slot = running + woff + inc - c;
#pragma unroll
    for (int i = 0; i < IRLE_E; ++i)
      if (v[i + 1] != v[i]) {
        if (slot < (unsigned)cap) out[slot] = (unsigned int)(j0 + i);
        ++slot;
      }
    __syncthreads();
    if (tid == 0) running += total;
    __syncthreads();
  }
#undef IRLE_AT
  const unsigned int nchg = running;          // runs = nchg + 1 (the first run counts zeros, possibly 0 of them)
  if (tid == 0) nruns[k] = nchg + 1 <= (unsigned)cap ? (int)(nchg + 1) : -(int)(nchg + 1);
  if (nchg + 1 > (unsigned)cap) return;
  // positions -> run lengths, in place, from the last chunk down (chunk c needs the last position of chunk c-1)
  if (tid == 0) out[nchg] = (unsigned int)len - (nchg ? out[nchg - 1] : 0u);
  __syncthreads();
  for (long hi = nchg; hi > 0; hi -= IRLE_T) {
    const long i = hi - 1 - tid;
    unsigned int cur = 0, prev = 0;
    if (i >= 0) { cur = out[i]; prev = i > 0 ? out[i - 1] : 0u; }
    __syncthreads();
    if (i >= 0) out[i] = cur - prev;
    __syncthreads();
  }
}

int rsis_l_palette_to_ids(const unsigned char* rgb, long npix, const unsigned char* table, int ntab, unsigned char* ids, hipStream_t st) {
  long gx = (npix + 255) / 256;
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(palette_to_ids_kernel, dim3((unsigned)gx), dim3(256), 0, st, rgb, npix, table, ntab, ids);
  return rsis_check_launch();
}

int rsis_l_idmap_rle_encode(const unsigned char* idmap, int h, int w, const int* ids, int k, unsigned int* counts, int cap, int* nruns,
                            hipStream_t st) {
  hipLaunchKernelGGL(idmap_rle_kernel, dim3(k), dim3(IRLE_T), 0, st, idmap, h, w, ids, counts, cap, nruns);
  return rsis_check_launch();
}
