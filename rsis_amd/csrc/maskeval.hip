// COCO 'segm' evaluation on the device (gfx950): what the reference's (modified) pycocotools COCOeval does per image and category on
// the host from run-length strings (reference src/coco/PythonAPI/pycocotools/cocoeval.py:164-191 computeIoU -> maskApi.c:77-96 rleIou,
// cocoeval.py:236-314 evaluateImg), restated on bit-packed masks.  All arithmetic up to the IoU division is integer, so nothing
// depends on the order of execution.
//   mask_pack_bits_kernel : uint8 0/1 masks [n][len] -> 64-bit words [n][stride] (element e is bit e % 64 of word e / 64, tail bits
//     zero) + area.  HBM-bound: 64 bytes in, 8 out per thread.
//   rle_to_bits_kernel    : run counts (rsis_rle_encode's / the decoded COCO text form) -> the same words; one block per mask: a
//     block scan turns counts into run ends, then every output word finds its first run by bisection and walks the runs it spans.
//   mask_intersect_kernel : grouped over the images of a call; inter[d][g] = sum_w popcount(dt[d][w] & gt[g][w]).  A block owns an
//     8 x 4 (detection x ground truth) tile over a chunk of 2048 words: per thread and 16-byte column the 4 ground-truth cells stay
//     in registers while the 8 detection cells stream past, so a tile pair reads each word once.  Chunks add into a zeroed
//     output with integer atomics (order-independent).
//   coco_iou_kernel       : per (image, category) cell the float64 IoU matrix of its score-sorted, truncated detections:
//     inter / (iscrowd ? area_d : area_d + area_g - inter), 0 where the masks do not meet (maskApi.c:93-94).
//   coco_match_kernel     : the greedy matching of evaluateImg, one wave per (image, category, area range) cell and one lane per
//     IoU threshold; the lanes of a wave read the same IoU (a broadcast) and write consecutive outputs.
#include "common.h"
#include "launchers.h"

typedef unsigned long long u64;

#define PB_T 256
// grid = (ceil(stride / 256), n): one output word per thread
__global__ __launch_bounds__(PB_T) void mask_pack_bits_kernel(const unsigned char* __restrict__ masks, long len, u64* __restrict__ bits,
                                                              long stride, unsigned int* __restrict__ area) {
  const int k = blockIdx.y;
  const long w = blockIdx.x * (long)PB_T + threadIdx.x;
  u64 word = 0;
  if (w < stride) {
    const long e0 = w * 64;
    const unsigned char* p = masks + (size_t)k * len + e0;
    if (e0 + 64 <= len && (((uintptr_t)p) & 15) == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 v = reinterpret_cast<const uint4*>(p)[q];
        const unsigned int x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned int y = x[j] | (x[j] >> 4);                  // any bit of a byte -> its bit 0 (shifts of 4 + 2 + 1 stay inside the byte)
          y |= y >> 2;
          y |= y >> 1;
          const unsigned int nib = (((y & 0x01010101u) * 0x01020408u) >> 24) & 0xFu;   // byte i -> bit i
          word |= (u64)nib << (16 * q + 4 * j);
        }
      }
    } else {
      for (int i = 0; i < 64; ++i)
        if (e0 + i < len && p[i]) word |= 1ull << i;
    }
    bits[(size_t)k * stride + w] = word;
  }
  unsigned int c = (unsigned int)__popcll(word);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(area + k, c);
}

#define RB_T 256
#define RB_E 4
// desc[k] = {first count, number of counts, first word, words} of mask k (offsets into counts / ends and bits)
__global__ __launch_bounds__(RB_T) void rle_to_bits_kernel(const unsigned int* __restrict__ counts, const long long* __restrict__ desc,
                                                           long counts_len, unsigned int* __restrict__ ends, u64* __restrict__ bits,
                                                           long bits_len, unsigned int* __restrict__ area) {
  const int k = blockIdx.x;
  const long off = desc[4 * k], m = desc[4 * k + 1], boff = desc[4 * k + 2], stride = desc[4 * k + 3];
  if (off < 0 || m < 0 || off + m > counts_len || boff < 0 || stride < 0 || boff + stride > bits_len) return;   // (block-uniform)
  const unsigned int* cn = counts + off;
  unsigned int* en = ends + off;
  __shared__ unsigned int wsum[RB_T / 64];
  __shared__ unsigned int running;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) running = 0;
  __syncthreads();
  // ---- pass 1: ends[r] = counts[0] + ... + counts[r] ----
  for (long base = 0; base < m; base += RB_T * RB_E) {
    const long j0 = base + (long)tid * RB_E;
    unsigned int v[RB_E], c = 0;
#pragma unroll
    for (int i = 0; i < RB_E; ++i) { v[i] = j0 + i < m ? cn[j0 + i] : 0u; c += v[i]; }
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
    for (int i = 0; i < RB_T / 64; ++i) {
      const unsigned int s = wsum[i];
      if (i < wv) woff += s;
      total += s;
    }
    unsigned int e = running + woff + inc - c;
#pragma unroll
    for (int i = 0; i < RB_E; ++i) {
      e += v[i];
      if (j0 + i < m) en[j0 + i] = e;
    }
    __syncthreads();
    if (tid == 0) running += total;
    __syncthreads();                                              // (also orders the writes of `ends` before pass 2 reads them)
  }
  // ---- pass 2: one output word at a time; run r holds ones iff r is odd ----
  unsigned int pc = 0;
  for (long w = tid; w < stride; w += RB_T) {
    const u64 lo = (u64)w * 64, hi = lo + 64;
    long a = 0, b = m;                                            // first run whose end lies beyond lo
    while (a < b) {
      const long mid = (a + b) >> 1;
      if ((u64)en[mid] > lo) b = mid; else a = mid + 1;
    }
    u64 word = 0, pos = lo;
    for (long r = a; r < m && pos < hi; ++r) {
      const u64 e = (u64)en[r] < hi ? (u64)en[r] : hi;
      if ((r & 1) && e > pos) {
        const unsigned int n1 = (unsigned int)(e - pos);
        word |= (n1 == 64 ? ~0ull : ((1ull << n1) - 1ull)) << (pos - lo);
      }
      if (e > pos) pos = e;
    }
    bits[boff + w] = word;
    pc += (unsigned int)__popcll(word);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pc += __shfl_down(pc, o, 64);
  __syncthreads();
  if (lane == 0) wsum[wv] = pc;
  __syncthreads();
  if (tid == 0) area[k] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

#define IT_T 256
#define IT_D 8
#define IT_G 4
#define IT_ITERS 4
#define IT_CHUNK (IT_T * 2 * IT_ITERS)      // words of a mask row per block
// jobs[j] = {dt_off, gt_off, D, G, stride, out_off, block_begin, 0}: D x G masks of `stride` words (even; offsets even: 16-byte cells)
__global__ __launch_bounds__(IT_T) void mask_intersect_kernel(const u64* __restrict__ bits, long bits_len, const long long* __restrict__ jobs,
                                                              int njobs, unsigned int* __restrict__ inter, long inter_len) {
  const int b = blockIdx.x;
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {                                               // last job whose block_begin <= b
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[8 * (long)mid + 6] <= b) lo = mid; else hi = mid - 1;
  }
  const long long* J = jobs + 8 * (long)lo;
  const long dt_off = J[0], gt_off = J[1], D = J[2], G = J[3], stride = J[4], out_off = J[5];
  if (D < 1 || G < 1 || stride < 2 || ((dt_off | gt_off | stride) & 1) || dt_off < 0 || gt_off < 0 || dt_off + D * stride > bits_len ||
      gt_off + G * stride > bits_len || out_off < 0 || out_off + D * G > inter_len)
    return;                                                       // (block-uniform) a table that does not fit the buffers touches nothing
  const int nch = (int)((stride + IT_CHUNK - 1) / IT_CHUNK), ngt = (int)((G + IT_G - 1) / IT_G), ndt = (int)((D + IT_D - 1) / IT_D);
  int tb = b - (int)J[6];
  const int ch = tb % nch; tb /= nch;
  const int g0 = (tb % ngt) * IT_G, d0 = (tb / ngt) * IT_D;
  if (tb / ngt >= ndt) return;
  const u64* gp[IT_G];
  const u64* dp[IT_D];
#pragma unroll
  for (int g = 0; g < IT_G; ++g) gp[g] = bits + gt_off + (long)(g0 + g < G ? g0 + g : G - 1) * stride;
#pragma unroll
  for (int d = 0; d < IT_D; ++d) dp[d] = bits + dt_off + (long)(d0 + d < D ? d0 + d : D - 1) * stride;
  unsigned int acc[IT_D][IT_G];
#pragma unroll
  for (int d = 0; d < IT_D; ++d)
#pragma unroll
    for (int g = 0; g < IT_G; ++g) acc[d][g] = 0;
#pragma unroll
  for (int it = 0; it < IT_ITERS; ++it) {
    const long w = (long)ch * IT_CHUNK + (long)it * (IT_T * 2) + threadIdx.x * 2;
    if (w < stride) {                                             // stride is even: w + 1 < stride as well
      ulonglong2 gv[IT_G];
#pragma unroll
      for (int g = 0; g < IT_G; ++g) gv[g] = *reinterpret_cast<const ulonglong2*>(gp[g] + w);
#pragma unroll
      for (int d = 0; d < IT_D; ++d) {
        const ulonglong2 dv = *reinterpret_cast<const ulonglong2*>(dp[d] + w);
#pragma unroll
        for (int g = 0; g < IT_G; ++g) acc[d][g] += (unsigned int)(__popcll(dv.x & gv[g].x) + __popcll(dv.y & gv[g].y));
      }
    }
  }
  __shared__ unsigned int tile[IT_D * IT_G];
  if (threadIdx.x < IT_D * IT_G) tile[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int d = 0; d < IT_D; ++d)
#pragma unroll
    for (int g = 0; g < IT_G; ++g) {
      unsigned int v = acc[d][g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tile[d * IT_G + g], v);
    }
  __syncthreads();
  if (threadIdx.x < IT_D * IT_G) {
    const int d = d0 + threadIdx.x / IT_G, g = g0 + threadIdx.x % IT_G;
    const unsigned int v = tile[threadIdx.x];
    if (d < D && g < G && v) atomicAdd(inter + out_off + (long)d * G + g, v);
  }
}

// cells[c] = {dt_begin, D, gt_begin, G, inter_off, inter_ld, iou_off, 0}; dt_row / dt_marea are indexed dt_begin + d (detections in
// score order), gt_col / gt_marea / gt_crowd gt_begin + g; ious[iou_off + d * G + g]
__global__ __launch_bounds__(64) void coco_iou_kernel(const long long* __restrict__ cells, const unsigned int* __restrict__ inter, long inter_len,
                                                      const int* __restrict__ dt_row, const unsigned int* __restrict__ dt_marea, long ndt,
                                                      const int* __restrict__ gt_col, const unsigned int* __restrict__ gt_marea,
                                                      const int* __restrict__ gt_crowd, long ngt, double* __restrict__ ious, long ious_len) {
  const long long* C = cells + 8 * (long)blockIdx.x;
  const long db = C[0], D = C[1], gb = C[2], G = C[3], ioff = C[4], ld = C[5], ooff = C[6];
  if (D < 1 || G < 1 || db < 0 || db + D > ndt || gb < 0 || gb + G > ngt || ooff < 0 || ooff + D * G > ious_len || ioff < 0 || ld < 1) return;
  for (long p = threadIdx.x; p < D * G; p += 64) {
    const long d = p / G, g = p - d * G;
    const long ii = ioff + (long)dt_row[db + d] * ld + gt_col[gb + g];
    if (ii < 0 || ii >= inter_len) continue;
    const unsigned int i = inter[ii], ad = dt_marea[db + d], ag = gt_marea[gb + g];
    const unsigned int u = gt_crowd[gb + g] ? ad : ad + ag - i;
    ious[ooff + p] = i == 0 ? 0.0 : (double)i / (double)u;
  }
}

#define MT_WAVES 4
// cells[c] = {iou_off, D, G, dt_begin, gt_begin, dt_out, gt_out, area range}: ious[iou_off + d * G + gperm[gt_begin + g]] is the IoU of
// detection d and the g-th ground truth in ignored-last order; gflag[gt_begin + g] = ignore | iscrowd << 1 in that order; dt_area is
// indexed dt_begin + d.  Outputs (lane = threshold t): dtm / dti [dt_out + d][T], gtm [gt_out + g][T] (zeroed by the caller); a match
// is stored as the partner's position in the cell's order + 1.
__global__ __launch_bounds__(64 * MT_WAVES) void coco_match_kernel(const long long* __restrict__ cells, int ncells, const double* __restrict__ ious,
                                                                   long ious_len, const int* __restrict__ gperm, const int* __restrict__ gflag,
                                                                   long ngt, const double* __restrict__ dt_area, long ndt,
                                                                   const double* __restrict__ arng, int nrng, const double* __restrict__ thrs, int T,
                                                                   int* __restrict__ dtm, int* __restrict__ dti, long dt_out_len,
                                                                   int* __restrict__ gtm, long gt_out_len) {
  const int c = blockIdx.x * MT_WAVES + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (c >= ncells || t >= T) return;
  const long long* C = cells + 8 * (long)c;
  const long ioff = C[0], D = C[1], G = C[2], db = C[3], gb = C[4], dout = C[5], gout = C[6], a = C[7];
  if (D < 0 || G < 0 || db < 0 || db + D > ndt || gb < 0 || gb + G > ngt || dout < 0 || dout + D > dt_out_len || gout < 0 ||
      gout + G > gt_out_len || a < 0 || a >= nrng || ioff < 0 || ioff + D * G > ious_len)
    return;
  const double thr = thrs[t] < 1.0 - 1e-10 ? thrs[t] : 1.0 - 1e-10, alo = arng[2 * a], ahi = arng[2 * a + 1];
  for (long d = 0; d < D; ++d) {
    double iou = thr;
    long m = -1;
    for (long g = 0; g < G; ++g) {
      const int fl = gflag[gb + g];
      if (gtm[(gout + g) * T + t] > 0 && !(fl & 2)) continue;    // matched already, and not a crowd
      if (m > -1 && !(gflag[gb + m] & 1) && (fl & 1)) break;     // holds a regular match: the ignored tail cannot replace it
      const double v = ious[ioff + d * G + gperm[gb + g]];
      if (v < iou) continue;
      iou = v;                                                    // (>=: among equal IoUs the last one wins)
      m = g;
    }
    int ig;
    if (m >= 0) {
      ig = gflag[gb + m] & 1;
      gtm[(gout + m) * T + t] = (int)d + 1;
    } else {
      const double ar = dt_area[db + d];
      ig = (ar < alo || ar > ahi) ? 1 : 0;
    }
    dtm[(dout + d) * T + t] = (int)m + 1;
    dti[(dout + d) * T + t] = ig;
  }
}

int rsis_l_mask_pack_bits(const unsigned char* masks, int n, long len, u64* bits, long stride, unsigned int* area, hipStream_t st) {
  if (rsis_zero_async(area, sizeof(unsigned int) * (size_t)n, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(mask_pack_bits_kernel, dim3((unsigned)((stride + PB_T - 1) / PB_T), n), dim3(PB_T), 0, st, masks, len, bits, stride, area);
  return rsis_check_launch();
}

int rsis_l_rle_to_bits(const unsigned int* counts, long counts_len, const long long* desc, int n, unsigned int* ends, u64* bits, long bits_len,
                       unsigned int* area, hipStream_t st) {
  if (rsis_zero_async(area, sizeof(unsigned int) * (size_t)n, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(rle_to_bits_kernel, dim3(n), dim3(RB_T), 0, st, counts, desc, counts_len, ends, bits, bits_len, area);
  return rsis_check_launch();
}

long rsis_l_mask_intersect_blocks(long D, long G, long stride) {
  return ((D + IT_D - 1) / IT_D) * ((G + IT_G - 1) / IT_G) * ((stride + IT_CHUNK - 1) / IT_CHUNK);
}

int rsis_l_mask_intersect_batch(const u64* bits, long bits_len, const long long* jobs, int njobs, int total_blocks, unsigned int* inter,
                                long inter_len, hipStream_t st) {
  if (rsis_zero_async(inter, sizeof(unsigned int) * (size_t)inter_len, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(mask_intersect_kernel, dim3(total_blocks), dim3(IT_T), 0, st, bits, bits_len, jobs, njobs, inter, inter_len);
  return rsis_check_launch();
}

int rsis_l_coco_iou_batch(const long long* cells, int ncells, const unsigned int* inter, long inter_len, const int* dt_row,
                          const unsigned int* dt_marea, long ndt, const int* gt_col, const unsigned int* gt_marea, const int* gt_crowd, long ngt,
                          double* ious, long ious_len, hipStream_t st) {
  hipLaunchKernelGGL(coco_iou_kernel, dim3(ncells), dim3(64), 0, st, cells, inter, inter_len, dt_row, dt_marea, ndt, gt_col, gt_marea, gt_crowd,
                     ngt, ious, ious_len);
  return rsis_check_launch();
}

int rsis_l_coco_match_batch(const long long* cells, int ncells, const double* ious, long ious_len, const int* gperm, const int* gflag, long ngt,
                            const double* dt_area, long ndt, const double* arng, int nrng, const double* thrs, int T, int* dtm, int* dti,
                            long dt_out_len, int* gtm, long gt_out_len, hipStream_t st) {
  if (gt_out_len > 0 && rsis_zero_async(gtm, sizeof(int) * (size_t)gt_out_len * T, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(coco_match_kernel, dim3((ncells + MT_WAVES - 1) / MT_WAVES), dim3(64 * MT_WAVES), 0, st, cells, ncells, ious, ious_len, gperm,
                     gflag, ngt, dt_area, ndt, arng, nrng, thrs, T, dtm, dti, dt_out_len, gtm, gt_out_len);
  return rsis_check_launch();
}

// host: the COCO text form -> counts (inverse of rsis_rle_to_string; maskApi.c:218-230); returns the number of counts, or -(number
// of counts) when cap is too small
int rsis_l_rle_from_string(const char* s, unsigned int* counts, int cap) {
  int m = 0;
  long p = 0;
  while (s[p]) {
    long x = 0;
    int k = 0, more = 1;
    while (more) {
      const long c = (long)s[p] - 48;
      if (s[p] == 0) { more = 0; break; }                         // (a truncated string ends the count where it stands)
      x |= (c & 0x1f) << (5 * k);
      more = (c & 0x20) != 0;
      ++p;
      ++k;
      if (!more && (c & 0x10)) x |= (long)(~0UL << (5 * k));
    }
    if (m > 2) x += (m - 2 < cap) ? (long)counts[m - 2] : 0;
    if (m < cap) counts[m] = (unsigned int)x;
    ++m;
  }
  return m <= cap ? m : -m;
}
