// eval --display figures on the device (gfx950): what the reference does per image on the host with matplotlib (reference
// src/eval.py:30-95 display_masks: every kept instance mask painted over the image in its sequence colour at opacity 0.5, the class
// name at the mask's centre of mass).  The masks already lie on the device as bytes, COLUMN-major (element x * h + y), where
// rsis_mask_resize_threshold wrote them; the image is ROW-major interleaved RGB.
//   overlay_masks_kernel: a block owns a tile of OV_TY rows x OV_TX columns.  Per painted mask it reads the tile with loads that are
//     contiguous along h (one 128-byte column segment per 8 lanes on the 16-byte path), parks it in LDS and reads it back transposed,
//     so that the lanes of a half wave hold 32 neighbouring pixels of an image ROW: the mask reads and the RGB loads / stores are both
//     contiguous across lanes.  Every thread keeps the running fp32 value of its 16 pixels x 3 channels in registers across the k masks;
//     the next masks' tiles (8 on the wide paths) are in flight in registers while one is blended.  Memory-bound: k * h * w mask bytes + 6 * h * w.
//   overlay_moments_kernel: (set pixels, sum of row indices, sum of column indices) per painted mask, integer sums in 64 bits: per-thread
//     partials, wave shuffles, LDS, one 64-bit atomic add per block and moment -- nothing depends on the order of execution.
#include "common.h"
#include "launchers.h"

#define OV_TY 128            // tile rows (contiguous mask bytes per column)
#define OV_TX 32             // tile columns (contiguous RGB pixels per row)
#define OV_T 256             // threads per block: thread t blends column t % 32, rows 16 * (t / 32) .. + 15
#define OV_PY 16             // pixels (rows) per thread
#define OV_PITCH 33          // LDS dwords per tile column: 32 of data + 1, so that 32 lanes reading 32 columns hit 32 banks
#define OV_MC 32             // moments: columns per block
#define OV_KC 256            // colours staged in LDS at a time

template <int V> struct ov_vec;
template <> struct ov_vec<1> { typedef unsigned char type; };
template <> struct ov_vec<4> { typedef unsigned int type; };
template <> struct ov_vec<16> { typedef uint4 type; };

// one tile of mask `m` into registers: unit u = pass * OV_T + t covers V rows of one column.  Every load is unconditional, from a clamped
// address (V > 1: h % V == 0, so y < h means y + V <= h): a load under a lane condition becomes a branch with a full wait for ALL
// outstanding loads behind it, which serialises the prefetches.  What a unit outside the image (or an order entry outside [0, n), which
// reads mask 0) brings in is never used: such pixels are not stored, such a mask is not blended.
template <int V>
__device__ __forceinline__ void ov_fetch(const unsigned char* __restrict__ masks, int m, int n, int h, int w, int y0, int x0,
                                         typename ov_vec<V>::type (&r)[OV_PY / V]) {
  typedef typename ov_vec<V>::type vec_t;
  constexpr int UPC = OV_TY / V;                      // units per tile column
  const unsigned char* base = masks + (size_t)(m >= 0 && m < n ? m : 0) * h * w;
#pragma unroll
  for (int p = 0; p < OV_PY / V; ++p) {
    const int u = p * OV_T + threadIdx.x;
    const int x = x0 + u / UPC, y = y0 + (u % UPC) * V;
    r[p] = *reinterpret_cast<const vec_t*>(base + (size_t)(x < w ? x : w - 1) * h + (y < h ? y : 0));
  }
}

template <int V>
__device__ __forceinline__ void ov_park(unsigned int* tile, const typename ov_vec<V>::type (&r)[OV_PY / V]) {
  constexpr int UPC = OV_TY / V;
#pragma unroll
  for (int p = 0; p < OV_PY / V; ++p) {
    const int u = p * OV_T + threadIdx.x;
    const int cx = u / UPC, yy = (u % UPC) * V;
    if constexpr (V == 1) {
      reinterpret_cast<unsigned char*>(tile)[cx * (OV_PITCH * 4) + yy] = r[p];
    } else if constexpr (V == 4) {
      tile[cx * OV_PITCH + yy / 4] = r[p];
    } else {
      unsigned int* d = tile + cx * OV_PITCH + yy / 4;
      d[0] = r[p].x; d[1] = r[p].y; d[2] = r[p].z; d[3] = r[p].w;
    }
  }
}

// grid = tiles_x * tiles_y blocks (tiles_x fastest)
template <int V>
__global__ __launch_bounds__(OV_T) void overlay_masks_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ masks,
                                                            int n, const int* __restrict__ order, const unsigned char* __restrict__ colors,
                                                            int k, float alpha, unsigned char* __restrict__ out, int h, int w, int tiles_x) {
  typedef typename ov_vec<V>::type vec_t;
  __shared__ unsigned int tile[2][OV_TX * OV_PITCH];
  const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * OV_TX, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * OV_TY;
  const int cx = threadIdx.x & (OV_TX - 1), g = threadIdx.x / OV_TX;
  const int x = x0 + cx, yb = y0 + g * OV_PY;
  const bool col_ok = x < w;

  float v[OV_PY][3];
#pragma unroll
  for (int i = 0; i < OV_PY; ++i) {
    const bool ok = col_ok && yb + i < h;
    const unsigned char* px = image + ((size_t)(ok ? yb + i : 0) * w + (ok ? x : 0)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[i][c] = (float)px[c];   // (a pixel outside the image reads pixel 0 and is never stored: no load under a condition)
  }

  // PF masks' tiles in flight per block, in registers (4 VGPRs each on the wide paths; a 1024 x 2048 image gives a CU only two blocks)
  constexpr int PF = V == 1 ? 2 : 8;
  // The colours come through LDS, OV_KC masks' worth at a time, staged BEFORE the prefetches are issued: the vector memory counter retires
  // in order, so a colour loaded from global memory inside the loop would make every blend wait for the prefetch issued just before it
  __shared__ unsigned char lcol[3 * OV_KC];
  for (int i = threadIdx.x; i < 3 * (k < OV_KC ? k : OV_KC); i += OV_T) lcol[i] = colors[i];
  vec_t r[PF][OV_PY / V] = {};
#pragma unroll
  for (int u = 0; u < PF; ++u)
    if (u < k) ov_fetch<V>(masks, order[u], n, h, w, y0, x0, r[u]);
  for (int j0 = 0; j0 < k; j0 += PF) {
    if (j0 > 0 && j0 % OV_KC == 0) {                   // (k > OV_KC only) the next OV_KC colours; PF divides OV_KC
      __syncthreads();
      for (int i = threadIdx.x; i < 3 * (k - j0 < OV_KC ? k - j0 : OV_KC); i += OV_T) lcol[i] = colors[3 * j0 + i];
    }                                                  // (the barrier of the first mask below orders these writes before their reads)
#pragma unroll
   for (int u = 0; u < PF; ++u) {
    const int j = j0 + u;
    if (j >= k) break;                                 // (uniform over the block)
    unsigned int* tl = tile[u & 1];                    // PF is even: u & 1 == j & 1
    ov_park<V>(tl, r[u]);
    const int mj = order[j];
    const bool painted = mj >= 0 && mj < n;            // (uniform) an order entry outside [0, n) paints nothing
    // (two buffers, one barrier per mask: a thread that parks mask j + 2 into this buffer has passed the barrier of mask j + 1,
    //  which every thread reaches only after it has read mask j)
    __syncthreads();
    if (j + PF < k) ov_fetch<V>(masks, order[j + PF], n, h, w, y0, x0, r[u]);
    const int jc = 3 * (j % OV_KC);
    const float c0 = (float)lcol[jc], c1 = (float)lcol[jc + 1], c2 = (float)lcol[jc + 2];
#pragma unroll
    for (int q = 0; q < OV_PY / 4; ++q) {
      const unsigned int bits = tl[cx * OV_PITCH + g * (OV_PY / 4) + q];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const bool on = painted && ((bits >> (8 * b)) & 0xffu) != 0u;
        float* pv = v[4 * q + b];
        pv[0] = on ? __builtin_fmaf(alpha, c0 - pv[0], pv[0]) : pv[0];
        pv[1] = on ? __builtin_fmaf(alpha, c1 - pv[1], pv[1]) : pv[1];
        pv[2] = on ? __builtin_fmaf(alpha, c2 - pv[2], pv[2]) : pv[2];
      }
    }
   }
  }

#pragma unroll
  for (int i = 0; i < OV_PY; ++i) {
    if (col_ok && yb + i < h) {
      unsigned char* px = out + ((size_t)(yb + i) * w + x) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = (unsigned char)(v[i][c] + 0.5f);
    }
  }
}

__device__ __forceinline__ unsigned long long ov_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// grid = (ceil(w / OV_MC), k): block (bx, j) sums columns bx * OV_MC .. + OV_MC - 1 of mask order[j], a contiguous range of the mask's
// bytes, in units of V rows (V > 1: h % V == 0); up to four loads of a thread are independent and in flight together
template <int V>
__global__ __launch_bounds__(OV_T) void overlay_moments_kernel(const unsigned char* __restrict__ masks, int n, const int* __restrict__ order,
                                                              int h, int w, unsigned long long* __restrict__ moments) {
  typedef typename ov_vec<V>::type vec_t;
  const int j = blockIdx.y, m = order[j];
  if (m < 0 || m >= n) return;                         // (uniform over the block; the moments of such an entry stay zero)
  const unsigned char* base = masks + (size_t)m * h * w;
  const int xa = blockIdx.x * OV_MC, xb = xa + OV_MC < w ? xa + OV_MC : w;
  const unsigned int upc = (unsigned int)(h / V);      // units per column
  const long units = (long)(xb - xa) * upc;
  const unsigned char* first = base + (size_t)xa * h;
  unsigned long long cnt = 0, sy = 0, sx = 0;
#pragma unroll 4
  for (long u = threadIdx.x; u < units; u += OV_T) {
    const vec_t bits = *reinterpret_cast<const vec_t*>(first + u * V);
    unsigned char b8[V];
    __builtin_memcpy(b8, &bits, V);
    const unsigned int cx = (unsigned int)(u / upc);
    const unsigned int y = (unsigned int)(u - (long)cx * upc) * V;
    unsigned int c = 0, ys = 0;                        // set pixels of this unit and how far they lie below its first row (< 16 * 16)
#pragma unroll
    for (int b = 0; b < V; ++b) {
      const unsigned int on = b8[b] != 0 ? 1u : 0u;
      c += on;
      ys += on * b;
    }
    cnt += c;
    sy += (unsigned long long)c * y + ys;
    sx += (unsigned long long)c * (unsigned int)(xa + cx);
  }
  __shared__ unsigned long long red[OV_T / 64][3];
  cnt = ov_wave_sum(cnt); sy = ov_wave_sum(sy); sx = ov_wave_sum(sx);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = cnt; red[threadIdx.x >> 6][1] = sy; red[threadIdx.x >> 6][2] = sx; }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
#pragma unroll
    for (int i = 0; i < OV_T / 64; ++i) t += red[i][threadIdx.x];
    if (t) atomicAdd(moments + (size_t)j * 3 + threadIdx.x, t);
  }
}

int rsis_l_overlay_moments(const unsigned char* masks, int n, const int* order, int k, int h, int w, unsigned long long* moments,
                           hipStream_t st) {
  if (rsis_zero_async(moments, sizeof(unsigned long long) * 3 * (size_t)k, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  const dim3 grid((unsigned)rsis_cdiv(w, OV_MC), (unsigned)k);
  if (h % 16 == 0 && ((uintptr_t)masks & 15) == 0)
    hipLaunchKernelGGL(overlay_moments_kernel<16>, grid, dim3(OV_T), 0, st, masks, n, order, h, w, moments);
  else if (h % 4 == 0 && ((uintptr_t)masks & 3) == 0)
    hipLaunchKernelGGL(overlay_moments_kernel<4>, grid, dim3(OV_T), 0, st, masks, n, order, h, w, moments);
  else
    hipLaunchKernelGGL(overlay_moments_kernel<1>, grid, dim3(OV_T), 0, st, masks, n, order, h, w, moments);
  return rsis_check_launch();
}

int rsis_l_overlay_masks(const unsigned char* image, const unsigned char* masks, int n, const int* order, const unsigned char* colors, int k,
                         float alpha, unsigned char* out, int h, int w, hipStream_t st) {
  const int tiles_x = rsis_cdiv(w, OV_TX);
  const long tiles = (long)tiles_x * rsis_cdiv(h, OV_TY);
  if (tiles > 0x7FFFFFFFL) return RSIS_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)tiles), blk(OV_T);
  const uintptr_t a = (uintptr_t)masks;
  if (k > 0 && h % 16 == 0 && (a & 15) == 0)
    hipLaunchKernelGGL(overlay_masks_kernel<16>, grid, blk, 0, st, image, masks, n, order, colors, k, alpha, out, h, w, tiles_x);
  else if (k > 0 && h % 4 == 0 && (a & 3) == 0)
    hipLaunchKernelGGL(overlay_masks_kernel<4>, grid, blk, 0, st, image, masks, n, order, colors, k, alpha, out, h, w, tiles_x);
  else
    hipLaunchKernelGGL(overlay_masks_kernel<1>, grid, blk, 0, st, image, masks, n, order, colors, k, alpha, out, h, w, tiles_x);
  return rsis_check_launch();
}
