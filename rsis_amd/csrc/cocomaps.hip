// Instance-id and class-id maps of a batch of COCO samples, painted on the device from the bit rows of their records (polymask.hip
// rsis_poly_to_bits / maskeval.hip rsis_rle_to_bits) at the OUTPUT size of the data layer: the host's per-instance decode, full-image
// compare and nearest zoom, flip and crop of two label images become one launch, and the label images never exist at native size.
//   The resize, flip and crop of a sample are two index tables, src_y[Ho] and src_x[Wo] (dataloader/coco.py builds them in float64 by
//   scipy's rule); the kernel does no floating-point arithmetic.  Output pixel (i, j) of sample b looks up bit src_x * h + src_y of
//   every record of the sample that still can win: the record of the SMALLEST area[] that covers the pixel wins, equal areas go to the
//   lower record index (the scan runs in index order and replaces the winner only for a strictly smaller area).
//   paint_maps_kernel: one block of 256 threads per 32 x 32 output tile.
//     stage : the sample's <= 255 records go to LDS once (thread r checks record r against the buffer lengths; a record that does not
//             fit gets area 0, which never wins).
//     probe : the rows are column-major (y fastest), so lanes run along y: lane l of a wave reads row l % 32 of columns l / 32, and
//             neighbouring lanes hit the same or the adjacent 64-bit word.  Four passes cover the tile's 32 columns.
//     store : the winners turn through a 32 x 33 LDS tile; lanes then run along x and write ins and seg with one 16-byte store each
//             per four pixels (Wo % 4 == 0 and 16-byte aligned outputs; element stores otherwise).
//   Integer compares only, no atomics, no workspace: the result does not depend on the order of execution.  Bound: the record scan
//   (one 8-byte L1 / L2 hit per record and pixel that is not ruled out by its area); HBM traffic is 8 B written per pixel.
#include <stdint.h>

#include "common.h"
#include "launchers.h"

typedef unsigned long long u64;

#define CM_T 256
#define CM_TILE 32
#define CM_MAXREC 255

// recs[r] = {first word, words, h, w, instance id, class id, 0, 0}; imgs[b] = {first record, records}
__global__ __launch_bounds__(CM_T) void paint_maps_kernel(const u64* __restrict__ bits, long bits_len, const unsigned int* __restrict__ area,
                                                          long nrec, const long long* __restrict__ recs, const long long* __restrict__ imgs,
                                                          int max_recs, const int* __restrict__ src_y, const int* __restrict__ src_x, int Ho,
                                                          int Wo, int tiles_x, int* __restrict__ ins, int* __restrict__ seg, int vec) {
  __shared__ long long r_fw[CM_MAXREC + 1];
  __shared__ int r_h[CM_MAXREC + 1], r_w[CM_MAXREC + 1], r_id[CM_MAXREC + 1], r_cls[CM_MAXREC + 1];
  __shared__ unsigned int r_area[CM_MAXREC + 1];
  __shared__ int win[CM_TILE][CM_TILE + 1];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int ty0 = (int)(blockIdx.x / tiles_x) * CM_TILE, tx0 = (int)(blockIdx.x % tiles_x) * CM_TILE;
  const long long first = imgs[2 * (long)b];
  long long cnt = imgs[2 * (long)b + 1];
  if (first < 0 || cnt < 0 || cnt > max_recs || cnt > CM_MAXREC || first > nrec || cnt > nrec - first) cnt = 0;   // (block-uniform)
  const int n = (int)cnt;
  if (tid < n) {
    const long long* R = recs + 8 * (first + tid);
    const long long fw = R[0], words = R[1], h = R[2], w = R[3], id = R[4], cls = R[5];
    const bool ok = fw >= 0 && words >= 0 && h >= 1 && w >= 1 && h < (1LL << 31) && w < (1LL << 31) && h * w < (1LL << 31) &&
                    words >= (h * w + 63) / 64 && fw <= bits_len && words <= bits_len - fw && id >= 1 && id <= 255 &&
                    cls >= INT32_MIN && cls <= INT32_MAX;
    r_fw[tid] = ok ? fw : 0;
    r_h[tid] = ok ? (int)h : 0;
    r_w[tid] = ok ? (int)w : 0;
    r_id[tid] = ok ? (int)id : 0;
    r_cls[tid] = ok ? (int)cls : 0;
    r_area[tid] = ok ? area[first + tid] : 0u;                    // a record that does not fit the buffers never wins
  }
  __syncthreads();
  // ---- probe: lanes along y ----
  {
    const int ly = tid & (CM_TILE - 1), lx0 = tid >> 5;
    const int i = ty0 + ly;
    const int sy = i < Ho ? src_y[(long)b * Ho + i] : -1;
#pragma unroll
    for (int p = 0; p < CM_TILE / (CM_T / CM_TILE); ++p) {
      const int lx = lx0 + p * (CM_T / CM_TILE);
      const int j = tx0 + lx;
      const int sx = j < Wo ? src_x[(long)b * Wo + j] : -1;
      int best = -1;
      unsigned int ba = 0xffffffffu;
      if (sy >= 0 && sx >= 0) {
        for (int r = 0; r < n; ++r) {
          const unsigned int a = r_area[r];
          if (a == 0u || a >= ba) continue;                       // (equal areas keep the lower index)
          const int h = r_h[r];
          if (sy >= h || sx >= r_w[r]) continue;
          const long e = (long)sx * h + sy;
          const u64 word = bits[r_fw[r] + (e >> 6)];
          if ((word >> (e & 63)) & 1ull) { best = r; ba = a; }
        }
      }
      win[ly][lx] = best;
    }
  }
  __syncthreads();
  // ---- store: lanes along x ----
  int* ib = ins + (long)b * Ho * Wo;
  int* sb = seg + (long)b * Ho * Wo;
  if (vec) {
    const int row = tid >> 3, c4 = (tid & 7) * 4;
    const int i = ty0 + row, j = tx0 + c4;
    if (i < Ho && j < Wo) {                                       // Wo % 4 == 0: the four pixels are inside together
      int vi[4], vs[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = win[row][c4 + q];
        vi[q] = r < 0 ? 0 : r_id[r];
        vs[q] = r < 0 ? 0 : r_cls[r];
      }
      const long o = (long)i * Wo + j;
      *reinterpret_cast<int4*>(ib + o) = make_int4(vi[0], vi[1], vi[2], vi[3]);
      *reinterpret_cast<int4*>(sb + o) = make_int4(vs[0], vs[1], vs[2], vs[3]);
    }
  } else {
    const int col = tid & (CM_TILE - 1);
    const int j = tx0 + col;
#pragma unroll
    for (int p = 0; p < CM_TILE / (CM_T / CM_TILE); ++p) {
      const int row = (tid >> 5) + p * (CM_T / CM_TILE);
      const int i = ty0 + row;
      if (i < Ho && j < Wo) {
        const int r = win[row][col];
        const long o = (long)i * Wo + j;
        ib[o] = r < 0 ? 0 : r_id[r];
        sb[o] = r < 0 ? 0 : r_cls[r];
      }
    }
  }
}

int rsis_l_paint_instance_maps(const u64* bits, long bits_len, const unsigned int* area, long nrec, const long long* recs, const long long* imgs,
                               int B, int max_recs, const int* src_y, const int* src_x, int Ho, int Wo, int* ins, int* seg, hipStream_t st) {
  const int tiles_x = (Wo + CM_TILE - 1) / CM_TILE, tiles_y = (Ho + CM_TILE - 1) / CM_TILE;
  const int vec = (Wo % 4 == 0) && ((uintptr_t)ins % 16 == 0) && ((uintptr_t)seg % 16 == 0);
  hipLaunchKernelGGL(paint_maps_kernel, dim3((unsigned)((long)tiles_x * tiles_y), (unsigned)B), dim3(CM_T), 0, st, bits, bits_len, area, nrec,
                     recs, imgs, max_recs, src_y, src_x, Ho, Wo, tiles_x, ins, seg, vec);
  return rsis_check_launch();
}

// ---- the ignore map of a batch (--ignore_regions): crowd records, as bit rows, resampled through the same src_y / src_x tables ----
// ign[b][i][j] = 1 where ANY crowd record of sample b covers native pixel (src_y[i], src_x[j]) and the painted instance map holds no
// instance there (an outlined instance inside a crowd still counts), else 0.  One thread per output pixel, at most max_recs (<= 255,
// the loader keeps 16) records per sample read straight from the tables; integer compares only.  Every element of ign is written.
// crecs[r] = {first word, words, h, w, 0, 0, 0, 0}; imgs[b] = {first record, records}
__global__ __launch_bounds__(CM_T) void paint_ignore_kernel(const u64* __restrict__ bits, long bits_len, long nrec, const long long* __restrict__ crecs,
                                                            const long long* __restrict__ imgs, int max_recs, const int* __restrict__ src_y,
                                                            const int* __restrict__ src_x, int Ho, int Wo, const int* __restrict__ ins,
                                                            unsigned char* __restrict__ ign) {
  const int b = blockIdx.y;
  const long o = (long)blockIdx.x * CM_T + threadIdx.x;
  if (o >= (long)Ho * Wo) return;
  const int i = (int)(o / Wo), j = (int)(o - (long)i * Wo);
  const long long first = imgs[2 * (long)b];
  long long cnt = imgs[2 * (long)b + 1];
  if (first < 0 || cnt < 0 || cnt > max_recs || cnt > CM_MAXREC || first > nrec || cnt > nrec - first) cnt = 0;
  const int sy = src_y[(long)b * Ho + i], sx = src_x[(long)b * Wo + j];
  const long out = (long)b * Ho * Wo + o;
  unsigned char v = 0;
  if (sy >= 0 && sx >= 0 && ins[out] == 0) {
    for (int r = 0; r < (int)cnt && !v; ++r) {
      const long long* R = crecs + 8 * (first + r);
      const long long fw = R[0], words = R[1], h = R[2], w = R[3];
      const bool ok = fw >= 0 && words >= 0 && h >= 1 && w >= 1 && h < (1LL << 31) && w < (1LL << 31) && h * w < (1LL << 31) &&
                      words >= (h * w + 63) / 64 && fw <= bits_len && words <= bits_len - fw;
      if (!ok || sy >= h || sx >= w) continue;                   // (a record that does not fit the buffers covers nothing)
      const long e = (long)sx * h + sy;
      v = (unsigned char)((bits[fw + (e >> 6)] >> (e & 63)) & 1ull);
    }
  }
  ign[out] = v;
}

int rsis_l_paint_ignore_map(const u64* bits, long bits_len, long nrec, const long long* crecs, const long long* imgs, int B, int max_recs,
                            const int* src_y, const int* src_x, int Ho, int Wo, const int* ins, unsigned char* ign, hipStream_t st) {
  const long blocks = ((long)Ho * Wo + CM_T - 1) / CM_T;
  hipLaunchKernelGGL(paint_ignore_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(CM_T), 0, st, bits, bits_len, nrec, crecs, imgs, max_recs,
                     src_y, src_x, Ho, Wo, ins, ign);
  return rsis_check_launch();
}
