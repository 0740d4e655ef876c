// Cityscapes instance-level evaluation on the device (gfx950): the pixel counting behind AP / AP50% (definition: rsis_amd/cityscapes_eval.py;
// the benchmark's own script forms `gt == instID & pred` over the whole image once per ground-truth instance and prediction).  For every
// image of a call: gt = uint16 instance ids, lut = 65536-entry id -> slot table (slots 0 .. S-1), P bit-packed masks (rsis_mask_pack_bits'
// layout) ->
//     counts[p * S + s] = #{ i : bit i of mask p set and lut[gt[i]] == s }  (p < P),      counts[P * S + s] = #{ i : lut[gt[i]] == s }.
// Everything is an integer count added with integer atomics, so nothing depends on the schedule.
//   inst_presence_kernel : flags[id] = 1 for every id that occurs (plain byte stores of the same value: the race is benign), so that the
//     lut can be built without sorting 2 M pixels per image.
//   inst_overlap_kernel  : a job (image) is cut into chunks of IO_CHUNK pixels x groups of 64 masks; a block owns one (chunk, group).
//       1. the block reads its 32 KiB of gt with 16-byte loads (an image may start at any even byte: the cells are the aligned ones that
//          cover the chunk, one more than IO_CELLS when the start is not aligned), translates every pixel through the lut (ONE lookup for
//          a cell whose 8 pixels agree) and leaves the slots in LDS, sl[bit][word]: gt is read once per group of 64 masks.  Group 0 also
//          counts the slots themselves (row P, the histogram).
//       2. thread t owns the 64-bit word t of the chunk in every mask of the group: a zero word costs one compare (most are zero: a mask
//          is one connected component); a set bit reads its slot from LDS.
//     Counts are merged before they leave the CU, as in labeleval.hip (NOTES.md (6c) / (8b)): a lane keeps ONE open run (row, slot, count);
//     a closed run adds into a block-private window of (64 masks + histogram) x IO_WS slots of LDS; a slot outside the window adds directly
//     to the global table, one atomic per RUN; at the end the block adds the non-zero cells of its window, at most one global atomic per
//     cell and block.
#include "common.h"
#include "launchers.h"

typedef unsigned long long u64;

#define IO_T 256
#define IO_CELLS 2048                       // 16-byte cells (8 pixels) per chunk
#define IO_CHUNK (IO_CELLS * 8)             // pixels per chunk = IO_T words of 64
#define IO_WS 64                            // slots of the LDS window
#define IO_ROWS 65                          // 64 masks of a group + the histogram row
#define IO_IDS 65536
#define IO_JOB 16                           // int64 entries per job

__device__ __forceinline__ void io_flush(unsigned key, unsigned cnt, unsigned* win, unsigned* tab, long S, long row0, long P) {
  if (!cnt) return;
  const unsigned rl = key >> 16, s = key & 0xFFFFu;
  if (s < IO_WS) atomicAdd(&win[rl * IO_WS + s], cnt);
  else atomicAdd(tab + (rl == 64 ? P : row0 + rl) * S + s, cnt);
}

__device__ __forceinline__ void io_push(unsigned key, unsigned n, unsigned& cur, unsigned& cnt, unsigned* win, unsigned* tab, long S, long row0,
                                        long P) {
  if (key == cur) {
    cnt += n;
  } else {
    io_flush(cur, cnt, win, tab, S, row0, P);
    cur = key;
    cnt = n;
  }
}

// last job whose entry `col` (block_begin of this launch) is <= b
__device__ __forceinline__ const long long* io_find_job(const long long* __restrict__ jobs, int njobs, int col, int b) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[IO_JOB * (long)mid + col] <= b) lo = mid; else hi = mid - 1;
  }
  return jobs + IO_JOB * (long)lo;
}

// jobs[j] = {gt_off (bytes, even), npix, lut_off, bits_off (words), stride (words), P, S, counts_off, block_begin, presence block_begin, 0 ..}
// pool: 16-byte aligned, pool_len (bytes) a multiple of 16
__global__ __launch_bounds__(IO_T) void inst_presence_kernel(const unsigned char* __restrict__ pool, long pool_len, const long long* __restrict__ jobs,
                                                             int njobs, unsigned char* __restrict__ flags, long flags_len) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long* J = io_find_job(jobs, njobs, 9, b);
  const long gt_off = J[0], npix = J[1], lut_off = J[2];
  const long chunk = b - J[9];
  if (gt_off < 0 || (gt_off & 1) || npix < 1 || npix >= (1L << 32) || gt_off > pool_len - 2 * npix || lut_off < 0 ||
      lut_off > flags_len - IO_IDS || chunk < 0 || chunk >= (npix + IO_CHUNK - 1) / IO_CHUNK)
    return;                                                       // (block-uniform) a job that does not fit the buffers touches nothing
  unsigned char* F = flags + lut_off;
  const long pb = chunk * IO_CHUNK;
  const long nloc = npix - pb < IO_CHUNK ? npix - pb : IO_CHUNK;
  const long A = gt_off + 2 * pb, A0 = A & ~15L;
  const int e = (int)((A - A0) >> 1);
  unsigned last = 0xFFFFFFFFu;
  for (int c = tid; c < IO_CELLS + 1; c += IO_T) {
    const long a = A0 + 16L * c;
    if (a >= A + 2 * nloc) break;                                 // (a + 16 <= pool_len: a < the image's end <= pool_len, both multiples of 16 apart)
    const uint4 v = *reinterpret_cast<const uint4*>(pool + a);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long px = (long)c * 8 + k - e;
      const unsigned id = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
      if (px >= 0 && px < nloc && id != last) {
        F[id] = 1;
        last = id;
      }
    }
  }
}

__global__ __launch_bounds__(IO_T) void inst_overlap_kernel(const unsigned char* __restrict__ pool, long pool_len, const long long* __restrict__ jobs,
                                                            int njobs, const unsigned short* __restrict__ lut, long lut_len,
                                                            const u64* __restrict__ bits, long bits_len, unsigned int* __restrict__ counts,
                                                            long counts_len) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long* J = io_find_job(jobs, njobs, 8, b);
  const long gt_off = J[0], npix = J[1], lut_off = J[2], bits_off = J[3], stride = J[4], P = J[5], S = J[6], counts_off = J[7];
  const long tb = b - J[8];
  if (gt_off < 0 || (gt_off & 1) || npix < 1 || npix >= (1L << 32) || gt_off > pool_len - 2 * npix || lut_off < 0 || lut_off > lut_len - IO_IDS ||
      P < 0 || P >= (1L << 31) || S < 1 || S > 65535 || counts_off < 0 || counts_off > counts_len - (P + 1) * S || tb < 0)
    return;                                                       // (block-uniform) a job that does not fit the buffers touches nothing
  const long nwords = (npix + 63) >> 6, nchunks = (npix + IO_CHUNK - 1) / IO_CHUNK, ngroups = P ? (P + 63) >> 6 : 1;
  if (tb >= nchunks * ngroups) return;
  if (P && (bits_off < 0 || stride < nwords || stride >= (1L << 32) || bits_off > bits_len - P * stride)) return;
  const long group = tb / nchunks, chunk = tb - group * nchunks, row0 = group * 64;
  unsigned int* tab = counts + counts_off;
  const unsigned short* L = lut + lut_off;
  __shared__ unsigned short sl[64 * IO_T];                        // sl[bit * IO_T + word]: slot of pixel 64 * word + bit of the chunk
  __shared__ unsigned int win[IO_ROWS * IO_WS];
  for (int c = tid; c < IO_ROWS * IO_WS; c += IO_T) win[c] = 0;
  __syncthreads();
  const long pb = chunk * IO_CHUNK;
  const long nloc = npix - pb < IO_CHUNK ? npix - pb : IO_CHUNK;
  const long A = gt_off + 2 * pb, A0 = A & ~15L;
  const int e = (int)((A - A0) >> 1);
  const bool hist = group == 0;
  unsigned cur = 0, cnt = 0;
  for (int c = tid; c < IO_CELLS + 1; c += IO_T) {                // stage 1: gt -> slots
    const long a = A0 + 16L * c;
    if (a >= A + 2 * nloc) break;
    const uint4 v = *reinterpret_cast<const uint4*>(pool + a);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    const long px0 = (long)c * 8 - e;
    const bool uni = (v.x == (v.x & 0xFFFFu) * 0x00010001u) & (v.y == v.x) & (v.z == v.x) & (v.w == v.x);
    if (uni && px0 >= 0 && px0 + 8 <= nloc) {                     // 8 pixels of one id, all inside the chunk: one lookup
      const unsigned s = L[v.x & 0xFFFFu];
#pragma unroll
      for (int k = 0; k < 8; ++k) sl[((px0 + k) & 63) * IO_T + ((px0 + k) >> 6)] = (unsigned short)s;
      if (hist && s < S) io_push((64u << 16) | s, 8u, cur, cnt, win, tab, S, row0, P);
      continue;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long px = px0 + k;
      if (px < 0 || px >= nloc) continue;
      const unsigned s = L[(w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu];
      sl[(px & 63) * IO_T + (px >> 6)] = (unsigned short)s;
      if (hist && s < S) io_push((64u << 16) | s, 1u, cur, cnt, win, tab, S, row0, P);
    }
  }
  __syncthreads();
  const long gp = P - row0 < 64 ? P - row0 : 64;                  // masks of this group (0 when P == 0)
  const long wd = chunk * IO_T + tid;
  if (gp > 0 && wd < nwords) {                                    // stage 2: word `tid` of the chunk in every mask of the group
    const long left = nloc - 64L * tid;                           // (>= 1) pixels of the image in this word
    const u64 valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    const u64* bp = bits + bits_off + row0 * stride + wd;
    for (int p0 = 0; p0 < gp; p0 += 8) {
      u64 m[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) m[u] = p0 + u < gp ? bp[(long)(p0 + u) * stride] : 0ull;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        u64 x = m[u] & valid;
        while (x) {
          const int i = __builtin_ctzll(x);
          x &= x - 1;
          const unsigned s = sl[i * IO_T + tid];
          if (s < S) io_push(((unsigned)(p0 + u) << 16) | s, 1u, cur, cnt, win, tab, S, row0, P);
        }
      }
    }
  }
  io_flush(cur, cnt, win, tab, S, row0, P);
  __syncthreads();
  for (int c = tid; c < IO_ROWS * IO_WS; c += IO_T) {
    const unsigned v = win[c];
    if (v) {
      const long rl = c / IO_WS, s = c % IO_WS;
      atomicAdd(tab + (rl == 64 ? P : row0 + rl) * S + s, v);     // (s < S: only slots below S were pushed)
    }
  }
}

long rsis_l_inst_overlap_blocks(long npix, long P) { return ((npix + IO_CHUNK - 1) / IO_CHUNK) * (P ? (P + 63) / 64 : 1); }

int rsis_l_inst_presence_batch(const unsigned char* pool, long pool_len, const long long* jobs, int njobs, int total_blocks, unsigned char* flags,
                               long flags_len, hipStream_t st) {
  if (rsis_zero_async(flags, (size_t)flags_len, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(inst_presence_kernel, dim3(total_blocks), dim3(IO_T), 0, st, pool, pool_len, jobs, njobs, flags, flags_len);
  return rsis_check_launch();
}

int rsis_l_inst_overlap_batch(const unsigned char* pool, long pool_len, const long long* jobs, int njobs, int total_blocks,
                              const unsigned short* lut, long lut_len, const u64* bits, long bits_len, unsigned int* counts, long counts_len,
                              hipStream_t st) {
  if (rsis_zero_async(counts, sizeof(unsigned int) * (size_t)counts_len, st) != RSIS_OK) return RSIS_ERR_LAUNCH;
  hipLaunchKernelGGL(inst_overlap_kernel, dim3(total_blocks), dim3(IO_T), 0, st, pool, pool_len, jobs, njobs, lut, lut_len, bits, bits_len, counts,
                     counts_len);
  return rsis_check_launch();
}
