// COCO polygon segmentations -> bit-packed masks on the device (gfx950): what the reference's vendored mask API does on the host for
// every polygon annotation (reference src/coco/common/maskApi.c:161-201 rleFrPoly, then :44-70 rleMerge with intersect = 0 over the
// parts of a record), restated in a parallel form that yields the same mask bit for bit.  The output is the layout of
// rsis_mask_pack_bits / rsis_rle_to_bits (maskeval.hip): element e = x * h + y is bit e % 64 of word e / 64, tail bits zero.
//   rleFrPoly scales the vertices by 5 and rounds them, walks every edge of the closed polygon one point per unit step of its longer
//   axis (maskApi.c:169-180), and keeps, wherever the walk changes its x, one boundary position a = x * h + y (:184-193); the sorted
//   positions are the run boundaries of the mask (:195-199: equal positions cancel in pairs).  Hence: the mask is the PREFIX PARITY,
//   in element order, of the set of positions toggled an odd number of times.
//   poly_to_bits_kernel: one block per record, one part at a time.
//     walk : point d of edge j is a closed form of (j, d), so each lane computes any point and its predecessor on its own; a block
//            scan of the edges' point counts (256 edges at a time) assigns points to lanes.  A point whose x differs from its
//            predecessor's toggles one bit of the record's zeroed scratch row with a 64-bit atomic XOR (order-independent).
//     fill : in-word prefix XOR (six shift / XOR steps) + the parity of all earlier words (ballot per wave, LDS across waves, a
//            running carry across 256-word chunks); tail masked; ORed into the output row (the union of the parts); scratch re-zeroed.
//   Coordinates are double, evaluated in the C code's order with contraction off: (int)(ys + s * t + .5) must not become an fma.
//   A zero-length edge has s = 0 / 0; its single point has the x of both neighbours, so its y is never read (as in the C code).
#include "common.h"
#include "launchers.h"

#pragma clang fp contract(off)

typedef unsigned long long u64;

#define PM_T 256

// point d of the walk from (x0, y0) to (x1, y1): maskApi.c:170-179
struct pm_point { int u, v; };
__device__ __forceinline__ pm_point pm_edge_point(int xs, int ys, int xe, int ye, int d) {
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
  if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
  const double s = dx >= dy ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy;
  pm_point p;
  if (dx >= dy) {
    const int t = flip ? dx - d : d;
    p.u = t + xs;
    p.v = (int)(((double)ys + s * (double)t) + .5);
  } else {
    const int t = flip ? dy - d : d;
    p.v = t + ys;
    p.u = (int)(((double)xs + s * (double)t) + .5);
  }
  return p;
}

__device__ __forceinline__ int pm_edge_count(int xs, int ys, int xe, int ye) {
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  return (dx > dy ? dx : dy) + 1;
}

// recs[r] = {first part, parts, h, w, first word, words, 0, 0}; parts[p] = {first vertex, vertices}; xy[2 * v] = x, xy[2 * v + 1] = y
__global__ __launch_bounds__(PM_T) void poly_to_bits_kernel(const double* __restrict__ xy, long nverts, const long long* __restrict__ parts,
                                                            long nparts, const long long* __restrict__ recs, u64* __restrict__ scratch,
                                                            u64* __restrict__ bits, long bits_len, unsigned int* __restrict__ area) {
  const long long* R = recs + 8 * (long)blockIdx.x;
  const long p0 = R[0], np = R[1], h = R[2], w = R[3], boff = R[4], stride = R[5];
  if (p0 < 0 || np < 0 || p0 + np > nparts || h < 1 || w < 1 || h >= (1L << 31) || w >= (1L << 31) || h * w >= (1L << 31) || boff < 0 ||
      stride < (h * w + 63) / 64 || boff + stride > bits_len)
    return;                                                       // (block-uniform) a table that does not fit the buffers touches nothing
  const long total = h * w;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  u64* sc = scratch + boff;
  u64* out = bits + boff;
  __shared__ int vx[PM_T + 2], vy[PM_T + 2];                      // vertices e0 - 1 .. e0 + 256 of the chunk of edges e0 .. e0 + 255
  __shared__ u64 cum[PM_T];                                       // inclusive scan of the chunk's point counts
  __shared__ u64 wsum[PM_T / 64];
  __shared__ unsigned int wpar[PM_T / 64];
  for (long i = tid; i < stride; i += PM_T) { sc[i] = 0; out[i] = 0; }
  __syncthreads();
  for (long p = p0; p < p0 + np; ++p) {
    const long v0 = parts[2 * p], k = parts[2 * p + 1];
    if (v0 < 0 || k < 1 || v0 + k > nverts) continue;             // (block-uniform)
    // ---- walk: toggles of this part ----
    for (long e0 = 0; e0 < k; e0 += PM_T) {
      for (int i = tid; i < PM_T + 2; i += PM_T) {
        long vi = e0 - 1 + i;
        if (vi >= 0 && vi <= k) {
          if (vi == k) vi = 0;                                    // the polygon closes back to vertex 0
          vx[i] = (int)(5.0 * xy[2 * (v0 + vi)] + .5);
          vy[i] = (int)(5.0 * xy[2 * (v0 + vi) + 1] + .5);
        }
      }
      __syncthreads();
      const u64 c = e0 + tid < k ? (u64)pm_edge_count(vx[tid + 1], vy[tid + 1], vx[tid + 2], vy[tid + 2]) : 0ull;
      u64 inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      u64 woff = 0;
#pragma unroll
      for (int i = 0; i < PM_T / 64; ++i)
        if (i < wv) woff += wsum[i];
      cum[tid] = woff + inc;
      __syncthreads();
      const u64 npts = cum[PM_T - 1];
      for (u64 q = tid; q < npts; q += PM_T) {
        int a = 0, b = PM_T - 1;                                  // first edge of the chunk whose inclusive count lies beyond q
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (cum[mid] > q) b = mid; else a = mid + 1;
        }
        const int d = (int)(q - (a ? cum[a - 1] : 0ull));
        if (e0 + a == 0 && d == 0) continue;                      // the first point of the walk has no predecessor
        const pm_point pt = pm_edge_point(vx[a + 1], vy[a + 1], vx[a + 2], vy[a + 2], d);
        const int b0 = d > 0 ? a + 1 : a;                         // the predecessor: on this edge, or the previous edge's last point
        const int bd = d > 0 ? d - 1 : pm_edge_count(vx[a], vy[a], vx[a + 1], vy[a + 1]) - 1;
        const pm_point pr = pm_edge_point(vx[b0], vy[b0], vx[b0 + 1], vy[b0 + 1], bd);
        if (pt.u == pr.u) continue;
        double xd = (double)(pt.u < pr.u ? pt.u : pt.u - 1);      // maskApi.c:185-189
        xd = (xd + .5) / 5.0 - .5;
        if (floor(xd) != xd || xd < 0 || xd > (double)(w - 1)) continue;
        double yd = (double)(pt.v < pr.v ? pt.v : pr.v);
        yd = (yd + .5) / 5.0 - .5;
        if (yd < 0) yd = 0; else if (yd > (double)h) yd = (double)h;
        yd = ceil(yd);
        const long pos = (long)(int)xd * h + (long)(int)yd;       // y == h: the first element of the next column
        if (pos < total) atomicXor(sc + (pos >> 6), 1ull << (pos & 63));
      }
      __syncthreads();                                            // vx / vy / cum are rewritten by the next chunk
    }
    // ---- fill: prefix parity of the toggles, ORed into the record's row ----
    unsigned int carry = 0;                                       // parity of all toggles before this chunk of words (block-uniform)
    for (long base = 0; base < stride; base += PM_T) {
      const long i = base + tid;
      u64 x = i < stride ? __hip_atomic_load(sc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;   // (written by atomics)
      const unsigned int par = (unsigned int)__popcll(x) & 1u;
      const u64 ball = __ballot(par);
      if (lane == 0) wpar[wv] = (unsigned int)__popcll(ball) & 1u;
      __syncthreads();
      unsigned int before = carry ^ ((unsigned int)__popcll(ball & ((1ull << lane) - 1ull)) & 1u), all = 0;
#pragma unroll
      for (int j = 0; j < PM_T / 64; ++j) {
        if (j < wv) before ^= wpar[j];
        all ^= wpar[j];
      }
      x ^= x << 1;
      x ^= x << 2;
      x ^= x << 4;
      x ^= x << 8;
      x ^= x << 16;
      x ^= x << 32;
      if (before) x = ~x;
      if (i < stride) {
        const long e = i * 64;
        const u64 keep = e + 64 <= total ? ~0ull : (e >= total ? 0ull : ((1ull << (total - e)) - 1ull));
        out[i] |= x & keep;
        sc[i] = 0;
      }
      carry ^= all;
      __syncthreads();                                            // wpar is rewritten; the zeroed scratch precedes the next part's toggles
    }
  }
  unsigned int pc = 0;
  for (long i = tid; i < stride; i += PM_T) pc += (unsigned int)__popcll(out[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pc += __shfl_down(pc, o, 64);
  if (lane == 0) wpar[wv] = pc;
  __syncthreads();
  if (tid == 0) {
    unsigned int s = 0;
    for (int j = 0; j < PM_T / 64; ++j) s += wpar[j];
    area[blockIdx.x] = s;
  }
}

int rsis_l_poly_to_bits(const double* xy, long nverts, const long long* parts, long nparts, const long long* recs, int n, u64* scratch, u64* bits,
                        long bits_len, unsigned int* area, hipStream_t st) {
  if (rsis_zero_async(area, sizeof(unsigned int) * (size_t)n, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(poly_to_bits_kernel, dim3(n), dim3(PM_T), 0, st, xy, nverts, parts, nparts, recs, scratch, bits, bits_len, area);
  return rsis_check_launch();
}
