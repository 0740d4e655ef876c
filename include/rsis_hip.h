/* librsis_hip.so -- C ABI of the MI355X (gfx950) RSIS hot path.
 *
 * The reference (imatge-upc/rsis) has no FFI: its hot path sits behind PyTorch nn.Modules
 * (src/modules/clstm.py, model.py, vision.py) that dispatch to cuDNN/THCUNN.  This header is the drop-in
 * boundary one level below that module surface: every entry point replaces the torch op(s) cited next to
 * it, on caller-owned device buffers, and is what the Python binding in rsis_amd/_lib.py (ctypes) loads.
 *
 * Conventions
 *   - every pointer is a device pointer to a caller-owned, contiguous fp32 NCHW tensor unless stated (also under
 *     RSIS_DTYPE_BF16: only the private packed weight copies are bf16);
 *   - no hidden allocation, no host synchronisation (one stated exception: rsis_targets_from_maps), graph-capture safe; work is
 *     enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return value: 0 = OK, nonzero = error code (rsis_error_string); nothing throws across the ABI;
 *   - thread-safe / re-entrant per stream.
 *   - "packed" weights are a private MFMA-friendly copy ([K rows][Cout padded to 128 columns]; K order and padding
 *     depend on the kernel that consumes them: implicit-GEMM (k = ci,r,s padded to 32 rows), direct 3x3 (8-channel
 *     chunks per concat source, channel pairs interleaved per tap) or bf16 cells (8 consecutive input channels per 16-byte
 *     cell, 16- / 64-channel chunks per concat source); ConvLSTM rows gate-interleaved 4*j+gate);
 *     they are rebuilt from the reference-layout weight ([Cout][Cin][k][k], gate order i,f,o,g) and never
 *     serialised.
 */
#ifndef RSIS_HIP_H
#define RSIS_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RSIS_ABI_VERSION 2

/* Arithmetic of the MFMA kernels behind the conv / ConvLSTM entry points (the `dtype` arguments below).
 *   RSIS_DTYPE_F32 : exact-f32 MFMA (v_mfma_f32_32x32x2_f32), bit-for-bit an fp32 fmaf chain.
 *   RSIS_DTYPE_BF16: operands rounded to bf16 (round-to-nearest-even) when they are staged, fp32 accumulation
 *                    (v_mfma_f32_32x32x16_bf16).  Tensors stay fp32 NCHW in memory; only the packed weight copy is bf16.
 *                    Layers without a bf16 kernel (the 7x7 stem, 3x3 / stride 2, the 8 -> 1 channel conv_out, odd-shaped weight
 *                    gradients) run their f32 kernel under either dtype; rsis_conv_uses_bf16 tells which. */
#define RSIS_DTYPE_F32 0
#define RSIS_DTYPE_BF16 1
/* rsis_conv2d_wgrad / rsis_wgrad_job.dtype only: dy and x are channel-blocked bf16 tensors (the "blk" layout of the entry points at
 * the end of this header), dW is fp32 in the reference layout as always; ks in {1, 3}, stride 1, "same" padding, Cout % 8 == 0 and
 * Cs % 8 == 0 (RSIS_ERR_UNSUPPORTED otherwise) */
#define RSIS_DTYPE_BF16_BLK 2
/* Exact-f32 arithmetic as RSIS_DTYPE_F32, but a 3x3 / stride 1 / pad 1 conv whose input AND output channel counts are multiples of 32
 * (one source, no ConvLSTM rows: rsis_conv_uses_wino) runs as Winograd F(2x2, 3x3) on the f32 MFMA (conv_wino.hip: 2.25x fewer
 * matrix flops, transforms fused into the staging path and the epilogue).  The packed copies then hold the TRANSFORMED weights
 * (G g G^T, 16 values per (output, input) channel pair); rsis_conv2d_fwd / _dgrad pick the kernel from this dtype.  Every other
 * geometry, and the weight gradient, behaves exactly as under RSIS_DTYPE_F32.  Results differ from the direct kernel by fp32
 * rounding only (measured closer to float64 than a sequential fp32 sum: the 2304-deep chain becomes 16 chains of 256). */
#define RSIS_DTYPE_F32_WINO 3
/* fp32 operands as RSIS_DTYPE_F32, but the TRAINING calls (rsis_conv2d_fwd with tile + 100, rsis_conv2d_dgrad, rsis_convlstm_fwd with
 * act_out, and their batch forms) of a 3x3 / stride 1 / pad 1 conv whose sources are multiples of 8 channels (data gradient: Cout % 8 == 0)
 * run on v_mfma_f32_32x32x16_bf16 with each operand split into three bf16 limbs (six of the nine limb products, those of weight
 * >= 2^-16, fp32 accumulation: conv3x3_limb.h).  The packed copies then hold the weight's three limbs (1.5 x the bytes of the f32 copy);
 * an inference call on such a copy returns RSIS_ERR_UNSUPPORTED (it belongs on the RSIS_DTYPE_F32 copy).  Every other geometry, and the
 * weight gradient, behaves exactly as under RSIS_DTYPE_F32.  Never split over K: one contributor per address in either mode. */
#define RSIS_DTYPE_F32_LIMB 4

int rsis_version(void);
const char* rsis_error_string(int code);
/* 1 when a conv of this geometry runs on the Winograd kernel under RSIS_DTYPE_F32_WINO */
int rsis_conv_uses_wino(int ks, int stride, int pad, int Cin, int Cout, int nseg, int lstm_hid);

/* Bit-reproducible mode (process-wide; initial value 1 when the environment has RSIS_DETERMINISTIC=1, else 0).  The reference's
 * CPU path is deterministic; this library's default is not: split-K sums, weight gradients and BatchNorm / bias / soft-IoU
 * reductions that span several blocks end in fp32 (fp64 for BatchNorm) atomics whose order varies run to run.  With the mode on
 * every such reduction has ONE contributor per address (no grid split-K, one block per reduced channel / dW tile, one wave per
 * soft-IoU image): same kernels, same results up to summation order, identical bits on every run -- at the price of launches
 * that no longer fill the chip.  Meant for debugging and for asserting graph replay == eager execution exactly.
 * rsis_set_deterministic returns the previous value. */
int rsis_set_deterministic(int on);
int rsis_get_deterministic(void);

/* ---- weight repacking (private cache of nn.Conv2d.weight; clstm.py:17, model.py:43-47,109, torchvision trunk) ---- */
/* 1 when a conv of this geometry runs on the bf16 kernels under RSIS_DTYPE_BF16 (3x3 / stride 1 / pad 1, and 1x1 / pad 0 -- the
 * strided 1x1 convs through their stride-1 form on a sub-sampled input -- with more than one output channel), 0 when it keeps
 * its f32 kernel and f32 packed layout */
int rsis_conv_uses_bf16(int ks, int stride, int pad, int Cout);
/* number of BYTES of the packed forward copy for a conv whose input is the channel concat of nseg tensors.
 * (dtype, ks, stride, pad) select the layout: bf16 cells, the direct-kernel layout (3x3/s1/p1, 3x3/s2/p1) or the implicit-GEMM one */
long rsis_conv_packed_bytes_fwd(int dtype, int Cout, int ks, int stride, int pad, int nseg, const int* Cseg);
/* number of BYTES of the packed dgrad copy producing c_count input channels */
long rsis_conv_packed_bytes_dgrad(int dtype, int Cout, int ks, int stride, int pad, int c_count);
/* The packed copy covers nseg (<= 3) input-channel segments of W: Cseg[s] channels starting at Coff[s] (Coff == NULL:
 * consecutive from 0) -- the channel concat the conv will gather from, or any subset of the input channels.
 * lstm_hid > 0: rows of W are [i|f|o|g] x hid (clstm.py:47) and are interleaved to 4*j+gate */
int rsis_conv_pack_fwd(const float* W, void* Wp, int Cout, int Ctot, int ks, int stride, int pad, int nseg, const int* Cseg,
                       const int* Coff, int lstm_hid, int dtype, void* stream);
/* dgrad copy: produces the gradient of the sum(Cseg) input channels of the segments (in segment order).  Both pack calls, the size
 * queries and rsis_conv_pack_job_fill follow ONE layout rule: like rsis_conv_pack_fwd, this call now returns RSIS_ERR_UNSUPPORTED for a
 * ConvLSTM weight (lstm_hid > 0) under RSIS_DTYPE_BF16 with ks != 3 (it used to pack it; no kernel reads such a copy) */
int rsis_conv_pack_dgrad(const float* W, void* Wd, int Cout, int Ctot, int ks, int stride, int pad, int nseg, const int* Cseg,
                         const int* Coff, int lstm_hid, int dtype, void* stream);

/* ---- nn.Conv2d forward (model.py:59-63 skip convs, :167 conv_out, vision.py:12-19 trunk convs) ----
 * out[B][Cout][Ho][Wo] = conv(cat(src[0..nsrc-1], dim=1), W, stride, pad) + bias (+ addend, same shape as out).
 * torch.cat (model.py:153) is folded in: up to 3 sources.  tile = 0 lets the library choose the MFMA tiling; tile + 100
 * additionally allows a split-K schedule (fp32 atomics: faster on deep-K / few-pixel layers such as sk5, but the summation
 * order is not reproducible -- the Python binding allows it only while training). */
int rsis_conv2d_fwd(const float* const* src, const int* Csrc, int nsrc, int B, int H, int W, const void* Wp, int Cout,
                    int ks, int stride, int pad, const float* bias, const float* addend, float* out, int Ho, int Wo,
                    int tile, int dtype, void* stream);
/* Inference: the conv above followed by the eval-mode nn.BatchNorm2d of its output (model.py:50-54,59-63; the bn1 / bn2 / bn3 /
 * downsample[1] of every torchvision Bottleneck behind vision.py:12-19), the residual add and the ReLU, in the conv's epilogue:
 *   out = relu?( (conv + bias - running_mean) / sqrt(running_var + eps) * gamma + beta  (+ addend) )
 * -- bit for bit what rsis_conv2d_fwd followed by rsis_bn_fwd(train = 0) writes (one shared definition of the arithmetic), without the
 * BatchNorm launch and its read + write of the activation.  fp32 kernels (dtype RSIS_DTYPE_F32, or a RSIS_DTYPE_BF16 pack of a conv the
 * library runs on the fp32 kernels anyway: the 7x7 stem), one destination, Cout % 4 == 0, no split-K (conv_out is not
 * covered): otherwise RSIS_ERR_UNSUPPORTED is returned BEFORE anything is launched and the caller runs the two launches. */
int rsis_conv2d_fwd_bn_eval(const float* const* src, const int* Csrc, int nsrc, int B, int H, int W, const void* Wp, int Cout,
                            int ks, int stride, int pad, const float* bias, const float* addend, const float* gamma, const float* beta,
                            const float* running_mean, const float* running_var, float eps, int relu, float* out, int Ho, int Wo,
                            int tile, int dtype, void* stream);

/* ---- nn.Conv2d backward-data (autograd of the above): dx for input channels [c_lo,c_hi) of the conv input, written
 * to ndst tensors dx[i] = [B][Cdx[i]][Hx][Wx] (the inverse of the channel concat). dy = [B][Cout][Hy][Wy].
 * Cin_packed = sum(Cseg) given to rsis_conv_pack_dgrad; sum(Cdx) <= Cin_packed (leading channels are produced).
 * addend (optional, ndst == 1): dx[0] = dgrad + addend -- the gradient the same tensor receives through another consumer (the
 * identity branch of a residual block), summed in the epilogue instead of by a separate pass.  stride 1: any pointer; 1x1 with
 * stride > 1: addend must BE dx[0] -- the strided gradient is accumulated into the existing tensor in place (no zero fill). ---- */
int rsis_conv2d_dgrad(const float* dy, int B, int Cout, int Hy, int Wy, const void* Wd, int Cin_packed, int ks, int stride,
                      int pad, float* const* dx, const int* Cdx, int ndst, int Hx, int Wx, const float* addend, int tile,
                      int dtype, void* stream);

/* ---- nn.Conv2d backward-weight: dW[Cout][Ctot][ks][ks] (reference layout) += corr(x, dy) for the source tensor
 * x = [B][Cs][H][W] that occupies input channels [c_off, c_off+Cs).  ACCUMULATES (fp32 atomics): zero dW first.
 * lstm_hid > 0: dy rows are gate-interleaved (4*j+gate) and are mapped back to reference rows. ---- */
int rsis_conv2d_wgrad(const float* dy, const float* x, float* dW, int B, int Cs, int H, int W, int Cout, int Ho, int Wo,
                      int ks, int stride, int pad, int Ctot, int c_off, int lstm_hid, int dtype, void* stream);

/* ---- many weight gradients in one call (same semantics as njobs calls of rsis_conv2d_wgrad, every dW ACCUMULATED; the dW regions
 * of different jobs may coincide -- e.g. the sources of one conv).  A weight gradient is off the critical path of the backward pass
 * (autograd of train.py:184 only needs it before the optimizer step), so the caller may park them and flush them here: the jobs that
 * run on the exact-f32 LDS-DMA tiled kernel are launched as ONE grid per tile configuration, sized for the whole set -- a layer on
 * its own must split its pixel axis 8-32 ways to fill the chip and pays a dW-sized pass of fp32 atomics per split.  The other jobs
 * are launched one by one.  The job array is host memory and is not referenced after the call returns. ---- */
typedef struct rsis_wgrad_job {
  const float* dy;     /* [B][Cout][Ho][Wo] */
  const float* x;      /* [B][Cs][H][W] */
  float* dW;           /* [Cout][Ctot][ks][ks], this source's channels start at c_off */
  int B, Cs, H, W, Cout, Ho, Wo, ks, stride, pad, Ctot, c_off, lstm_hid, dtype;
} rsis_wgrad_job;
int rsis_conv2d_wgrad_batch(const rsis_wgrad_job* jobs, int njobs, void* stream);

/* ---- conv bias gradient: db[Cout] += sum_{b,h,w} dy  (ACCUMULATES; lstm_hid as above) ---- */
int rsis_bias_grad(const float* dy, float* db, int B, int C, int HW, int lstm_hid, void* stream);

/* ---- ConvLSTMCell.forward (clstm.py:19-62): cat(x.., h_prev) -> Gates conv -> chunk -> sigmoid/tanh -> c,h in ONE
 * kernel.  src = the x tensor(s) followed by h_prev (omit h_prev and pass c_prev = NULL for the zero state of
 * clstm.py:26-37).  bias_packed / act_out / addend use interleaved rows.  act_out (post-nonlinearity i,f,o,g, needed
 * by the backward) may be NULL for inference. addend: optional precomputed time-invariant gate contribution (the
 * skip-feature part of the gate conv + bias, computed once per iteration by rsis_conv2d_fwd on interleaved rows); with an
 * addend nsrc may be 0 (level 0 at t = 0).  RSIS_DTYPE_BF16 covers ks == 3 only (RSIS_ERR_UNSUPPORTED otherwise, from
 * this call and from rsis_conv_pack_fwd with lstm_hid > 0): cells with another kernel size run under RSIS_DTYPE_F32. ---- */
int rsis_convlstm_fwd(const float* const* src, const int* Csrc, int nsrc, int B, int H, int W, const void* Wp,
                      const float* bias_packed, const float* addend, const float* c_prev, float* h_out, float* c_out,
                      float* act_out, int hid, int ks, int pad, int tile, int dtype, void* stream);

/* Several INDEPENDENT rsis_convlstm_fwd calls as ONE launch: the cells (level i, timestep d - i) of one diagonal of the decoder's
 * (level, timestep) wavefront -- level i at step t needs level i-1 at step t and itself at step t-1 (model.py:129-165 inside the
 * loop of train.py:85-94 / test.py:37-38), so the cells of a diagonal do not depend on each other.  Exact-f32 3x3 jobs share one
 * grid (conv3x3_direct_group_kernel: blocks of different jobs have different lengths and phases, so one job's prologue / epilogue
 * overlaps another's MFMA loop); other jobs, and every job in the deterministic mode, are launched one after the other -- the
 * results are those of njobs single calls either way (same kernels, same tiles, same summation order).  Fields as the arguments
 * of rsis_convlstm_fwd (src / Csrc hold nsrc <= 3 entries). */
typedef struct rsis_lstm_job {
  const float* src[3];
  int Csrc[3];
  int nsrc, B, H, W;
  const void* Wp;
  const float* bias_packed;
  const float* addend;
  const float* c_prev;
  float* h_out;
  float* c_out;
  float* act_out;
  int hid, ks, pad, tile, dtype;
  /* optional [B][hid] 64-bit keys, ZEROED by the caller: the global max-pool of h (model.py:143, the side feature) is then taken in
   * the kernel's epilogue -- every half wave adds its best (value, pixel) with an atomic max; key = order-preserving bits of the
   * value << 32 | (0x7FFFFFFF - flat pixel index); order-independent, so bit-reproducible.  rsis_heads_fwd_keys decodes them.
   * 3x3 gates only (RSIS_ERR_UNSUPPORTED otherwise). */
  unsigned long long* side_key;
} rsis_lstm_job;
int rsis_convlstm_fwd_batch(const rsis_lstm_job* jobs, int njobs, void* stream);

/* ---- ConvLSTMCell pointwise backward: (dh + dh2, dc_next, saved act, c_prev, c) -> da (gate pre-activation grads,
 * interleaved rows) and dc_prev.  dh / dh2 / dc_next / c_prev / dc_prev / da_sum may be NULL. da_sum += da if given.
 * dh2: the gradient reaching h through a second consumer (the next timestep's recurrence), summed in the kernel. ---- */
int rsis_convlstm_bwd_gates(const float* dh, const float* dh2, const float* dc_next, const float* act, const float* c_prev,
                            const float* c, float* da, float* dc_prev, float* da_sum, int B, int hid, int HW, void* stream);

/* Several INDEPENDENT rsis_convlstm_bwd_gates calls (da_sum == NULL) in one launch, and several independent rsis_conv2d_dgrad calls in
 * one launch where they run on the exact-f32 direct 3x3 kernel (stride 1, pad 1, no addend; other jobs, and every job in the
 * deterministic mode, are issued one by one): the cells (level i, timestep d - i) of a diagonal of the decoder's (level, timestep)
 * wavefront in the BACKWARD pass -- cell (i, t) needs d(up) from cell (i + 1, t) and (dh, dc) from cell (i, t + 1), both one diagonal
 * later, so the cells of a diagonal are independent (reference: autograd of model.py:129-165 inside train.py:85-94).  Fields as the
 * arguments of the single calls. */
typedef struct rsis_lstm_bwd_job {
  const float* dh;
  const float* dh2;
  const float* dc_next;
  const float* act;
  const float* c_prev;
  const float* c;
  float* da;
  float* dc_prev;
  int B, hid, HW;
} rsis_lstm_bwd_job;
int rsis_convlstm_bwd_gates_batch(const rsis_lstm_bwd_job* jobs, int njobs, void* stream);
typedef struct rsis_dgrad_job {
  const float* dy;
  int B, Cout, Hy, Wy;
  const void* Wd;
  int Cin_packed, ks, stride, pad;
  float* dx[3];
  int Cdx[3];
  int ndst, Hx, Wx;
  const float* addend;
  int tile, dtype;
} rsis_dgrad_job;
int rsis_conv2d_dgrad_batch(const rsis_dgrad_job* jobs, int njobs, void* stream);

/* ---- nn.UpsamplingBilinear2d(size) = bilinear, align_corners=True (model.py:149,163; train.py:96; test.py:39) ---- */
int rsis_upsample_bilinear_ac_fwd(const float* x, float* y, long BC, int Hi, int Wi, int Ho, int Wo, void* stream);
int rsis_upsample_bilinear_ac_bwd(const float* dy, float* dx, long BC, int Hi, int Wi, int Ho, int Wo, void* stream);
/* the two consumers of a level's hidden state besides the recurrence (model.py:143,149-150) back-propagated in one launch:
 * dx = upsample_backward(dy) + dpool[bc] at pixel argmax[bc] of every plane (argmax from rsis_global_maxpool_fwd) */
int rsis_upsample_maxpool_bwd(const float* dy, const float* dpool, const int* argmax, float* dx, long BC, int Hi, int Wi, int Ho,
                              int Wo, void* stream);

/* ---- nn.MaxPool2d(full map) side features (model.py:143): y[BC], argmax[BC] (int32 flat index) ---- */
int rsis_global_maxpool_fwd(const float* x, float* y, int* argmax, long BC, int HW, void* stream);
int rsis_global_maxpool_bwd(const float* dy, const int* argmax, float* dx, long BC, int HW, void* stream);
/* dx[bc][argmax[bc]] += dy[bc] (dx already holds the gradient of another consumer of the same tensor) */
int rsis_global_maxpool_bwd_add(const float* dy, const int* argmax, float* dx, long BC, int HW, void* stream);

/* ---- the decoder's dropout (model.py:137-182: nn.Dropout2d on every level's hidden state, nn.Dropout on the class / stop head
 * features), folded into the launches the decoder already makes.  Dropout2d is ONE factor s in {0, 1 / (1 - p)} per channel plane:
 * it commutes with the global max-pool (s >= 0) and with the bilinear resize, so no kernel ever forms the dropped hidden state.
 * `scale` below is [BC] fp32, one factor per plane; a NULL scale makes every call the unscaled entry point above, bit for bit.
 *   rsis_upsample_bilinear_ac_scaled_fwd : y = scale * resize(x): interpolated in fp32 as rsis_upsample_bilinear_ac_fwd does, then
 *                                          multiplied (equal sizes: the scaled copy);
 *   rsis_upsample_maxpool_scaled_bwd     : dx = scale * (resize^T(dy) + dpool at argmax);
 *   rsis_global_maxpool_scaled_bwd_add   : dx[bc][argmax[bc]] += scale[bc] * dy[bc];
 *   rsis_scale_planes                    : y[bc][:] = scale[bc] * x[bc][:] (HW elements per plane; x == y allowed): the transpose of
 *                                          the equal-size resize. ---- */
int rsis_upsample_bilinear_ac_scaled_fwd(const float* x, const float* scale, float* y, long BC, int Hi, int Wi, int Ho, int Wo, void* stream);
int rsis_upsample_maxpool_scaled_bwd(const float* dy, const float* dpool, const int* argmax, const float* scale, float* dx, long BC, int Hi,
                                     int Wi, int Ho, int Wo, void* stream);
int rsis_global_maxpool_scaled_bwd_add(const float* dy, const int* argmax, const float* scale, float* dx, long BC, int HW, void* stream);
int rsis_scale_planes(const float* x, const float* scale, float* y, long BC, int HW, void* stream);

/* ---- `-skip_mode mul` (model.py:156): level i >= 1 consumes resize(h[i-1]) * skip[i].
 *   rsis_upsample_bilinear_ac_mul_fwd : y = resize(x) * m, m [BC][Ho][Wo]: interpolated in fp32 as rsis_upsample_bilinear_ac_fwd does on
 *                                       the same launch paths, then ONE fp32 product per element.  Equal sizes: y = x * m.
 *   rsis_upsample_mul_bwd_prep        : the backward's preparation, one launch at the fine resolution.  With u = resize(x) recomputed
 *                                       (the unscaled forward's bits),
 *                                           dm[e] = accumulate ? fmaf(dy[e], u[e], dm[e]) : dy[e] * u[e]     (accumulate: 0 or 1)
 *                                           dy[e] = dy[e] * m[e]                                             (in place)
 *                                       after which rsis_upsample_maxpool_bwd / rsis_upsample_bilinear_ac_bwd run unchanged on dy.
 * Wo % 4 == 0: y, m, dy and dm must be 16-byte aligned. ---- */
int rsis_upsample_bilinear_ac_mul_fwd(const float* x, const float* m, float* y, long BC, int Hi, int Wi, int Ho, int Wo, void* stream);
int rsis_upsample_mul_bwd_prep(float* dy, const float* x, const float* m, float* dm, long BC, int Hi, int Wi, int Ho, int Wo, int accumulate,
                               void* stream);

/* The mask generator: ONE launch fills the three scale arrays of a whole sequence, n floats each,
 *   array 0 = s2 (Dropout2d, rate p2), array 1 = mc (class head, rate pc), array 2 = ms (stop head, rate ps),
 * all in the layout of the decoder's pooled side features: level after level, each [T][B][hid_i] (n = T * B * sum hid_i).
 * state: 8 device words (uint32), owned by the caller:
 *   state[0] = key word 0: the seed;   state[1] = key word 1: the rank of the process;
 *   state[2], state[3] = the call counter (low, high word);   state[4] = 0 between calls (the kernel's block ticket);  5..7 unused.
 * Element e (0 <= e < n) of array a is a pure function of (state, a, e):
 *   w[0..3] = Philox4x32-10(counter = (e >> 2, a, state[2], state[3]), key = (state[0], state[1]))     (Salmon et al., SC'11)
 *   word = w[e & 3];   u = (word >> 8) * 2^-24 (exact in fp32);   kept iff u >= p;
 *   value = kept ? 1.0f / (1.0f - p) (one fp32 division) : 0.0f            -- p == 0: all ones.
 * The kernel reads the state and then advances the call counter by one itself (an ordinary store by the last block to have read it), so a
 * captured graph draws fresh masks on every replay with no host involvement.  0 <= p < 1 for every rate, else RSIS_ERR_ARG (nothing
 * launched, the state untouched). */
int rsis_dropout_scales(unsigned int* state, float* s2, float* mc, float* ms, long n, float p2, float pc, float ps, void* stream);
/* The head masks, element-wise over the n pooled features (all arrays in the layout above):
 *   rsis_dropout_heads_mask     : side <- s2 * side (in place: SIDE = s2 * decode(KEY)), side_c = mc * side, side_s = ms * side -- the
 *                                 features the class / stop heads (rsis_heads_fwd / rsis_heads_wide_fwd) are then run on;
 *   rsis_dropout_heads_mask_bwd : dside = mc * dside_c + ms * dside_s (either gradient may be NULL = zero), from the d side of two
 *                                 rsis_heads_bwd / rsis_heads_wide_bwd calls (dstop == NULL on side_c, dprobs == NULL on side_s). */
int rsis_dropout_heads_mask(float* side, const float* s2, const float* mc, const float* ms, float* side_c, float* side_s, long n, void* stream);
int rsis_dropout_heads_mask_bwd(const float* dside_c, const float* dside_s, const float* mc, const float* ms, float* dside, long n, void* stream);

/* ---- nn.BatchNorm2d (+ residual add + ReLU of the bottleneck) (model.py:50-54,59-63; torchvision trunk) ----
 * train bit0: batch statistics, running-stat update (momentum, unbiased var), saves mean / rstd for the backward;
 * train bit1: `stats` (scratch of 2*C doubles) was zeroed by the caller (one memset for a whole arena instead of one per
 * layer). res may be NULL. */
int rsis_bn_fwd(const float* x, const float* res, float* y, double* stats, const float* gamma, const float* beta,
                float* running_mean, float* running_var, float* save_mean, float* save_rstd, int B, int C, int HW,
                float eps, float momentum, int relu, int train, void* stream);
/* train-mode backward. relu bit0: the forward applied ReLU (y, the forward output, is read for the mask); bit1: `stats`
 * was zeroed by the caller; bit2: ACCUMULATE into dgamma / dbeta instead of overwriting. dres (grad of the residual
 * input = masked dy) may be NULL. */
int rsis_bn_bwd(const float* dy, const float* x, const float* y, const float* save_mean, const float* save_rstd,
                const float* gamma, double* stats, float* dx, float* dres, float* dgamma, float* dbeta, int B, int C,
                int HW, int relu, void* stream);

/* eval-mode backward (the module in .eval(): y = relu?(gamma (x - running_mean) / sqrt(running_var + eps) + beta (+ res)), statistics are
 * constants): g = dy * [y > 0] if relu bit0, dx = gamma / sqrt(running_var + eps) * g, dres = g, dgamma = sum g xhat, dbeta = sum g.
 * Flags and scratch as rsis_bn_bwd (bit1: stats zeroed by the caller; bit2: accumulate into dgamma / dbeta). */
int rsis_bn_bwd_eval(const float* dy, const float* x, const float* y, const float* running_mean, const float* running_var,
                     const float* gamma, double* stats, float* dx, float* dres, float* dgamma, float* dbeta, int B, int C, int HW,
                     float eps, int relu, void* stream);

/* The same three with the ReLU mask of the forward output as bytes, for layers with ReLU and HW % 4 == 0 (RSIS_ERR_UNSUPPORTED
 * otherwise, before anything is launched: the caller keeps y and uses the three above).  ReLU is implied (no relu argument / bit0).
 * mask is [B*C*HW / 4] bytes: mask[i / 4] for the float4 group at flat NCHW element index i, bit k = (y[i + k] > 0) taken from
 * the value stored as y (NaN gives 0) -- the layout depends on the element index alone.  rsis_bn_fwd_mask writes y exactly as
 * rsis_bn_fwd(relu = 1) does, and the mask beside it; the backward entry points read the mask where the ones above read y (1 byte
 * instead of 16 per group) and write exactly what those write given that y.  flags: bit1 / bit2 as the relu argument above. */
int rsis_bn_fwd_mask(const float* x, const float* res, float* y, unsigned char* mask, double* stats, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float* save_mean, float* save_rstd, int B, int C, int HW,
                     float eps, float momentum, int train, void* stream);
int rsis_bn_bwd_mask(const float* dy, const float* x, const unsigned char* mask, const float* save_mean, const float* save_rstd,
                     const float* gamma, double* stats, float* dx, float* dres, float* dgamma, float* dbeta, int B, int C,
                     int HW, int flags, void* stream);
int rsis_bn_bwd_eval_mask(const float* dy, const float* x, const unsigned char* mask, const float* running_mean, const float* running_var,
                          const float* gamma, double* stats, float* dx, float* dres, float* dgamma, float* dbeta, int B, int C, int HW,
                          float eps, int flags, void* stream);

/* ---- y[bc][ho][wo] = x[bc][ho * stride][wo * stride], y is [BC][(H-1)/stride+1][(W-1)/stride+1]: the dense input of a
 * 1x1 / stride-s conv (torchvision Bottleneck downsample, layers 2-4; reference vision.py:16-19) -- x[:, :, ::s, ::s].contiguous().
 * The conv then runs as its stride-1 form (rsis_conv2d_fwd on y) and y is what its weight gradient reads. ---- */
int rsis_subsample2d(const float* x, float* y, long BC, int H, int W, int stride, void* stream);

/* ---- nn.MaxPool2d(3, stride 2, padding 1) of the ResNet stem (vision.py:15) ---- */
int rsis_maxpool3x3s2_fwd(const float* x, float* y, unsigned char* argmax, long BC, int H, int W, int Ho, int Wo,
                          void* stream);
/* accumulate != 0: dx += (dx already holds the gradient the pooled tensor's input receives from another consumer) */
int rsis_maxpool3x3s2_bwd(const float* dy, const unsigned char* argmax, float* dx, long BC, int H, int W, int Ho, int Wo,
                          int accumulate, void* stream);

/* ---- torch.optim.Adam step on a flat parameter range (utils/utils.py:83-84; train.py:185-187); g is scaled by gscale
 * (1/world_size after the RCCL sum all-reduce) before the L2 weight-decay term is added.  step: the 1-based update count of
 * the range (bias correction); step_dev != NULL: the count is read from that device int32 instead (the caller increments it on
 * the stream), so that a captured hipGraph replays with the live count. ---- */
int rsis_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, float gscale, const int* step_dev, void* stream);

/* ---- the other two rules of utils/utils.py:78-87 (-optim / -optim_cnn sgd, rmsprop) on a flat parameter range, with the same
 * gradient handling as rsis_adam_step: d = g * gscale + weight_decay * p.  Parameters without a gradient are the caller's to skip
 * (no range covers them).  n == 0 is a no-op.
 * torch.optim.SGD(momentum), dampening 0, no Nesterov: buf = momentum * buf + d; p -= lr * buf.  A zero-filled buf gives torch's first
 * step (buf = d), so no step count is kept; momentum 0 is plain SGD (p -= lr * d). ---- */
int rsis_sgd_step(float* p, const float* g, float* buf, long n, float lr, float momentum, float weight_decay, float gscale,
                  void* stream);
/* ---- torch.optim.RMSprop, no momentum, not centred: sq = alpha * sq + (1 - alpha) * d * d; p -= lr * d / (sqrt(sq) + eps). ---- */
int rsis_rmsprop_step(float* p, const float* g, float* sq, long n, float lr, float alpha, float eps, float weight_decay, float gscale,
                      void* stream);

/* ---- Hungarian matching of predictions to ground-truth slots (hungarian.py:91-125, munkres.Munkres().compute per
 * sample): scores[B][G][T] fp32 (rows = GT slots, columns = predictions, T <= G <= 128) -> perm[B][G] int64 with
 * perm[b][t] = GT slot of prediction t for t < T and 0 elsewhere.  Minimum total cost; runs on the device so the training
 * iteration needs no host synchronisation. ---- */
int rsis_assign_min_cost(const float* scores, long long* perm, int B, int G, int T, void* stream);

/* ---- batched repack: every packed weight copy of a model in ONE launch (after an optimizer step).  `jobs` is a DEVICE array
 * of njobs descriptors, sorted by block_begin; job i is processed by the blocks [block_begin_i, block_begin_{i+1}) of a grid
 * of total_blocks blocks, rsis_conv_pack_job_blocks() blocks each.  rsis_conv_pack_job_fill() fills the derived fields
 * (imode, ldw, krows) of a host-side descriptor exactly as rsis_conv_pack_fwd / _dgrad would choose them and returns the
 * job's block count (< 0: invalid). ---- */
typedef struct rsis_pack_job {
  const float* W;      /* reference-layout weight [Cout][Ctot][ks][ks] (device) */
  void* out;           /* packed copy (device), rsis_conv_packed_bytes_fwd / _dgrad bytes */
  int dgrad;           /* 0: forward copy, 1: data-gradient copy */
  int dtype;           /* RSIS_DTYPE_* of the kernels that will read the copy */
  int Cout, Ctot, ks, stride, pad, nseg, Cseg[3], Coff[3], lstm_hid;
  int imode, ldw, krows;   /* derived (rsis_conv_pack_job_fill) */
  int block_begin;     /* first block of this job in the batch grid */
} rsis_pack_job;
int rsis_conv_pack_job_fill(rsis_pack_job* job);
int rsis_conv_pack_batch(const rsis_pack_job* jobs_dev, int njobs, int total_blocks, void* stream);

/* ---- conv_out (nn.Conv2d(Cin, 1, 3, padding=1), model.py:109,167): weight AND bias gradient in one launch (the bias gradient is
 * the sum of dy, which the weight-gradient kernel reads anyway).  dy[B][1][H][W], x[B][Cin][H][W]; dW[Cin*9] (reference layout
 * [1][Cin][3][3]) and db[1] (may be NULL) are ACCUMULATED.  Cin in {4, 8, 16}, W % 4 == 0, else RSIS_ERR_UNSUPPORTED. ---- */
int rsis_conv_out_wgrad(const float* dy, const float* x, float* dW, float* db, int B, int Cin, int H, int W, void* stream);

/* ---- conv_out over ALL T timesteps of a decoded sequence in one launch each way (model.py:167 inside the loop of train.py:85-94:
 * out_mask_t = conv_out(upsampled hidden state of the last level at step t); the T applications are independent).  The Cin-channel
 * tensors are [T][B][Cin][H][W] (the decoder's stacked per-step buffers), the one-channel tensors are [B][T][H*W] -- the (B, T, N)
 * layout train.py:118 stacks the mask logits into, so no torch.stack copy is needed.  Same kernels and per-image arithmetic as
 * rsis_conv2d_fwd / _dgrad / rsis_conv_out_wgrad on one timestep.  Cin in {4, 8, 16}, W % 4 == 0, else RSIS_ERR_UNSUPPORTED.
 * Wp / Wd: the RSIS_DTYPE_F32 packs of conv_out's weight (rsis_conv_pack_fwd / _dgrad; conv_out keeps its f32 kernels under
 * RSIS_DTYPE_BF16); dW / db are ACCUMULATED. ---- */
int rsis_conv_out_seq_fwd(const float* x, const void* Wp, const float* bias, float* y, int T, int B, int Cin, int H, int W, void* stream);
int rsis_conv_out_seq_dgrad(const float* dy, const void* Wd, float* dx, int T, int B, int Cin, int H, int W, void* stream);
int rsis_conv_out_seq_wgrad(const float* dy, const float* x, float* dW, float* db, int T, int B, int Cin, int H, int W, void* stream);

/* ---- y[n] = sum_t x[t][n], t ascending (fixed order): sum over the timesteps of the stacked gate gradients, i.e. the gradient of a
 * ConvLSTM level's time-invariant gate term (autograd's accumulation over the T uses of the skip features, train.py:85-94) ---- */
int rsis_sum_leading(const float* x, float* y, int T, long n, void* stream);

/* ---- data-layer augmentation: nearest-neighbour affine warp (dataloader/transforms/utils.py:67-147 th_affine2d(mode='nearest',
 * center=True); applied by transforms.py:23-142 RandomAffine to the image, the instance map and the class map of a sample).
 * x, y: [N][C][H][W] float32 (y != x); mat: [N][mat_rows][3] float32 in DEVICE memory, mat_rows = 3 (the reference's 3x3, last
 * row ignored) or 2.  y[n][c][i][j] = x[n][c][round(clamp(A (i-ci, j-cj) + b + (ci, cj)))], ci = H/2 - 0.5, cj = W/2 - 0.5,
 * float32 arithmetic in the reference's operation order, round half to even: bit-exact with the reference. ---- */
int rsis_affine_nearest(const float* x, float* y, const float* mat, int mat_rows, int N, int C, int H, int W, void* stream);

/* ---- data-layer targets for a whole batch in one call (dataloader/dataset.py:86-146 sequence_from_masks + utils.batch_to_var):
 * ins, seg: [B][H][W] int32 instance-id / class-id maps; T = gt_maxseqlen.  Per image the smallest id PRESENT is the background and is
 * dropped; the other ids become rows ordered by area, largest first (equal areas: the larger id first), truncated to T:
 *   y_mask[B][T][H*W] fp32 = 1 where ins == the row's id (EVERY element is written: no memset is needed), y_class[B][T] int64 = the
 *   smallest seg value under the instance (0 on an empty row), sw_mask[B][T] fp32 = 1 on instance rows, sw_class[B][T] fp32 = 1 on
 *   instance rows and on the first empty row.
 * Integer counts and integer atomics only: the result does not depend on the order of execution.  work: caller-owned scratch of
 * rsis_targets_work_ints(B) int32.  Instance ids must lie in 0..255 (Pascal VOC, CVPPP); otherwise RSIS_ERR_UNSUPPORTED is returned and
 * no output has been written.  That test needs the histogram of the batch, so this call -- unlike the rest of the library --
 * synchronises `stream` once and must not be made during a stream capture.  H*W < 2^31, B <= 65535. ---- */
long rsis_targets_work_ints(int B);
int rsis_targets_from_maps(const int* ins, const int* seg, int B, int H, int W, int T, float* y_mask, long long* y_class, float* sw_mask,
                           float* sw_class, int* work, void* stream);

/* ---- Cityscapes label maps of a whole batch from the raw `*_instanceIds` values (dataloader/cityscapes.py:67-92):
 * raw: [B][H][W] int32; a value outside 0..65535 counts as 0.  class_of_label: [n_labels] int32 in DEVICE memory, n_labels <= 66.
 * Per pixel label = raw / 1000 and cls = class_of_label[label] if raw >= 1000 and label < n_labels, else 0; a pixel is KEPT when
 * cls > 0.  seg[B][H][W] = cls; ins[B][H][W] = 1 + the number of distinct kept raw values of image b that are smaller than this
 * pixel's, 0 on a pixel that is not kept -- the ranks np.unique gives, up to 65536 of them (a rank above 255 is written as it is:
 * rsis_targets_from_maps is the one that refuses it).  EVERY element of ins and seg is written.  work: caller-owned scratch of
 * rsis_instance_maps_work_ints(B) int32 (a 65536-bit presence bitmap per image), zeroed by the call itself.  No host sync, no
 * allocation, capture-safe; bitwise / integer atomics only, so the result does not depend on the order of execution.
 * H*W < 2^31, B <= 65535. ---- */
long rsis_instance_maps_work_ints(int B);
int rsis_instance_maps(const int* raw, const int* class_of_label, int n_labels, int B, int H, int W, int* ins, int* seg, int* work,
                       void* stream);

/* ---- Pascal VOC preparation (dataloader/pascal_precompute.py:36-101; dataset_utils.py convert_from_color_segmentation) ----
 * rsis_palette_to_ids: rgb[npix][3] uint8 -> ids[npix] uint8 through a colour table table[ntab][4] = (r, g, b, id) in DEVICE memory,
 *   ntab <= 256; the first matching entry wins, a colour that is not in the table maps to 0.
 * rsis_idmap_rle_encode: idmap[h][w] uint8 (ROW-major, as the .npy stores it) and k ids[k] (device, int32) -> the run counts of the k
 *   masks (idmap == ids[j]) in the COLUMN-major element order of rsis_rle_encode, one launch, without forming the k byte masks:
 *   counts[k][cap] / nruns[k] exactly as rsis_rle_encode writes them (nruns negative when cap is too small).  h*w < 2^32. */
int rsis_palette_to_ids(const unsigned char* rgb, long npix, const unsigned char* table, int ntab, unsigned char* ids, void* stream);
int rsis_idmap_rle_encode(const unsigned char* idmap, int h, int w, const int* ids, int k, unsigned int* counts, int cap, int* nruns,
                          void* stream);

/* ---- soft-IoU matching scores and matched-loss gradient (train.py:98-110,127-131,162-163; hungarian.py:62-89 softIoU) ----
 * rsis_softiou_sums: logits[B][T][N] (mask logits of the T predictions), y[B][G][N] (ground-truth masks, 0/1 floats) ->
 *   S[B][T+1][G+1]:  S[t][g] = sum_n sigmoid(logits[t][n]) * y[g][n],  S[t][G] = sum_n sigmoid(logits[t][n]),
 *   S[T][g] = sum_n y[g][n]  (S[T][G] is left 0).  One pass over both tensors; requires T <= 128, G <= 128, N % 8 == 0.
 *   The reference's cost is then 1 - S[t][g] / (S[t][G] + S[T][g] - S[t][g] + 1e-6) for every pair.
 * rsis_softiou_bwd: gradient of the matched costs w.r.t. the logits,
 *   dlogits[b][t][n] = (ca[b][t]*y + cb[b][t]*(1-y)) * p*(1-p),  y = y[b][perm[b*perm_ld + t]][n], p = sigmoid(logits[b][t][n]);
 *   the caller supplies ca = -g/U, cb = g*I/U^2 (g = upstream gradient of the cost, U = the cost's denominator). N % 4 == 0. */
int rsis_softiou_sums(const float* logits, const float* y, float* S, int B, int T, int G, long N, void* stream);
int rsis_softiou_bwd(const float* logits, const float* y, const long long* perm, int perm_ld, const float* ca, const float* cb,
                     float* dlogits, int B, int T, int G, long N, void* stream);
/* The same two with an IGNORE REGION: ignore[B][N], one byte per pixel, 0 = the pixel counts, non-zero = ignored (COCO crowds,
 *   Cityscapes groups); with k = (ignore == 0):  S[t][g] = sum_n k p y,  S[t][G] = sum_n k p,  S[T][g] = sum_n k y  (y is masked by the
 *   kernel, not by a promise of the caller), and dlogits is +0.0 at every ignored pixel.  An image ignored everywhere has S = 0: cost 1
 *   for every pair, zero gradient.  Same layout, limits, early returns and deterministic-mode launch plan as the plain entry points;
 *   ignore must be 4-byte aligned (RSIS_ERR_ARG otherwise); ignore == NULL IS the plain entry point (same kernel object, same bits). */
int rsis_softiou_sums_ignore(const float* logits, const float* y, const unsigned char* ignore, float* S, int B, int T, int G, long N,
                             void* stream);
int rsis_softiou_bwd_ignore(const float* logits, const float* y, const unsigned char* ignore, const long long* perm, int perm_ld,
                            const float* ca, const float* cb, float* dlogits, int B, int T, int G, long N, void* stream);

/* ---- class / stop heads of one decoder timestep (model.py:169-182): side = channel concat (by pointer) of nside <= 5 vectors
 * side[i][B][Cside[i]] (the global max-pools of the hidden states); class_probs[B][ncls] = softmax(Wc side + bc) with
 * Wc[ncls][K], K = sum Cside; stop[B] = Ws . side + bs (a logit).  rsis_heads_bwd: dside[i][B][Cside[i]] (any pointer may be
 * null) from dprobs[B][ncls] / dstop[B] (either may be null = zero), and dWc, dbc, dWs, dbs are ACCUMULATED into (null = skip).
 * K <= 2048, ncls <= 64; rsis_heads_bwd: 2 B (ncls + 1) + B ceil(K / B) floats of LDS <= 64 KB -- B = 320 rows at 21 classes (the parameter gradients are reduced over the rows in-kernel, no atomics; decoder_seq passes the T * B rows of all timesteps in one call). ---- */
int rsis_heads_fwd(const float* const* side, const int* Cside, int nside, int B, const float* Wc, const float* bc, int ncls,
                   const float* Ws, const float* bs, float* class_probs, float* stop, void* stream);
/* rsis_heads_fwd with the pooled side features given as the keys of rsis_lstm_job.side_key (one [B][Cside[i]] key array per level):
 * decodes them, ALSO writes the float features to side_out[i] and the arg-max pixels to arg_out[i] (what rsis_global_maxpool_fwd
 * would have produced: the backward passes read those), then computes the heads as rsis_heads_fwd does. */
int rsis_heads_fwd_keys(const unsigned long long* const* keys, float* const* side_out, int* const* arg_out, const int* Cside, int nside,
                        int B, const float* Wc, const float* bc, int ncls, const float* Ws, const float* bs, float* class_probs, float* stop,
                        void* stream);
int rsis_heads_bwd(const float* const* side, const int* Cside, int nside, int B, const float* Wc, int ncls, const float* Ws,
                   const float* class_probs, const float* dprobs, const float* dstop, float* const* dside, float* dWc, float* dbc,
                   float* dWs, float* dbs, void* stream);
/* The WIDE heads family: the same operation for 1 <= ncls <= 1024 and ANY rows >= 1 (1 <= K <= 2048, nside <= 5; anything else
 * RSIS_ERR_UNSUPPORTED, nothing written).  The callers use the three entry points above wherever those accept the call (the results of
 * the two families agree to rounding, not by bits: the softmax sum and the sums over the rows are taken in another order).
 * rsis_heads_wide_fwd: keys == NULL reads side[i] as rsis_heads_fwd does; otherwise keys / side_out / arg_out as rsis_heads_fwd_keys
 * (side is ignored).  The softmax is reduced by the whole block in a fixed order.
 * rsis_heads_wide_bwd: the semantics of rsis_heads_bwd (NULL dprobs / dstop = zero, NULL dside[i] / parameter targets skipped, the
 * parameter gradients ACCUMULATED) in two launches on `stream`, no atomics, bit-reproducible: a pass over the rows that leaves the
 * d-logits in scratch[rows][ncls + 1] and writes d side, then a pass over 16 x 64 tiles of the (ncls + 1) x K parameter gradient that
 * sums over the rows in a fixed order.  scratch: device floats, scratch_floats >= rows * (ncls + 1) (RSIS_ERR_ARG otherwise, nothing
 * written); it allocates nothing and can be captured into a graph. */
int rsis_heads_wide_fwd(const unsigned long long* const* keys, float* const* side_out, int* const* arg_out, const float* const* side,
                        const int* Cside, int nside, int rows, const float* Wc, const float* bc, int ncls, const float* Ws, const float* bs,
                        float* class_probs, float* stop, void* stream);
int rsis_heads_wide_bwd(const float* const* side, const int* Cside, int nside, int rows, const float* Wc, int ncls, const float* Ws,
                        const float* class_probs, const float* dprobs, const float* dstop, float* const* dside, float* dWc, float* dbc,
                        float* dWs, float* dbs, float* scratch, long scratch_floats, void* stream);

/* ---- loss tail of a training iteration (train.py:159-176; hungarian.py:10-59): masked means of the class NLL (probs[n][C],
 * targets y_class[n] int64, optional per-class weights cls_w[C]), of the matched soft-IoU costs siou[n] and of the balanced stop
 * BCE (logits stop[n], target = sw_mask, balance weight bw or < 0 = positives / n), n = B*T samples; sw_mask / sw_class are the
 * 0/1 sample weights.  out[4] = {w_iou*iou + w_cls*cls + w_stop*stop, iou, stop, cls} (pass w_cls / w_stop = 0 for a disabled
 * loss).  With dprobs / dstop / dsiou non-null the same launch also writes the gradient of out[0] * gout[0] (gout: device
 * pointer to the upstream gradient, null = 1) w.r.t. the three inputs (out may then be null). ---- */
int rsis_loss_tail(const float* probs, const long long* y_class, const float* stop, const float* siou, const float* sw_mask,
                   const float* sw_class, const float* cls_w, int n, int C, float bw, float w_iou, float w_cls, float w_stop,
                   float* out, float* dprobs, float* dstop, float* dsiou, const float* gout, void* stream);

/* ---- inference post-processing of predicted masks (eval.py:96-127 resize_mask + pycocotools mask.encode; RLE semantics of
 * src/coco/common/maskApi.c:32-41,196-209) ----
 * rsis_mask_resize_threshold: prob[n][Hm][Wm] fp32 -> seg[n][w][h] uint8 (COLUMN-major h x w masks: align-corners bilinear
 *   resample == scipy.ndimage.zoom(order=1), `> th`, pixels with ignore[h][w] == 1 cleared (ignore may be null)), the same
 *   without the ignore mask in raw (may be null), area[n] = number of set pixels of seg.
 * rsis_rle_encode: masks[n][len] uint8 column-major -> counts[n][cap] uint32 = lengths of the alternating runs starting with
 *   the (possibly empty) run of zeros; nruns[n] = number of runs, or -(number of runs) when cap is too small (counts then
 *   undefined for that mask).
 * rsis_rle_to_string: HOST function (host pointers): the COCO text form of `m` counts into out[cap]; returns its length
 *   (NUL-terminated) or -1 when cap is too small. */
int rsis_mask_resize_threshold(const float* prob, int n, int Hm, int Wm, const unsigned char* ignore, float th, unsigned char* seg,
                               unsigned char* raw, unsigned int* area, int h, int w, void* stream);
int rsis_rle_encode(const unsigned char* masks, int n, long len, unsigned int* counts, int cap, int* nruns, void* stream);
int rsis_rle_to_string(const unsigned int* counts, int m, char* out, int cap);
/* largest 8-connected component of n binary masks [n][h][w] (row-major, 0/1) -> out [n][h][w] (eval_cityscapes.py:131-150:
 * skimage.measure.label + most frequent label; ties: the component first in raster order).  Caller-owned workspaces:
 * labels[n*h*w], counts[n*h*w] int32, best[n] int32.  h*w < 2^31. */
int rsis_largest_component(const unsigned char* mask, unsigned char* out, int* labels, int* counts, int* best, int n, int h, int w,
                           void* stream);

/* ---- eval --display figures (eval.py:30-95 display_masks: the kept instance masks painted over the image in their sequence colours,
 * the class name at each mask's centre of mass; overlay.hip) ----
 * masks[n][w][h] uint8 are COLUMN-major h x w masks, zero / non-zero: the seg / raw layout of rsis_mask_resize_threshold.  order[k]
 * int32 (DEVICE) picks the k masks to draw and gives their paint order; an entry outside [0, n) cannot be checked without a copy and
 * paints nothing (its moments are zero).  h, w <= 2^30.
 * rsis_overlay_moments: moments[k][3] unsigned 64-bit = (set pixels, sum of row indices, sum of column indices) of mask order[j].
 *   Integer sums in 64 bits (the column sum passes 2^32 at 2048 x 4096): nothing depends on the order of execution.  k == 0: nothing
 *   is launched.
 * rsis_overlay_masks: image[h][w][3] and out[h][w][3] uint8, ROW-major interleaved RGB; colors[k][3] uint8 (DEVICE).  Per pixel and
 *   channel in fp32: v = image; for j = 0 .. k-1 in that order, where mask order[j] is non-zero at the pixel, v = fmaf(alpha,
 *   (float)colors[j][c] - v, v); out = (uint8)(v + 0.5f).  k == 0 copies the image (masks / order / colors may then be null); out may
 *   not alias image.
 * RSIS_ERR_ARG, nothing launched: a null pointer with k > 0 (image / out: always), n < 1 with k > 0, h or w < 1, k < 0, alpha outside
 *   [0, 1] (NaN included), out == image. */
int rsis_overlay_moments(const unsigned char* masks, int n, const int* order, int k, int h, int w, unsigned long long* moments,
                         void* stream);
int rsis_overlay_masks(const unsigned char* image, const unsigned char* masks, int n, const int* order, const unsigned char* colors,
                       int k, float alpha, unsigned char* out, int h, int w, void* stream);

/* ---- COCO 'segm' evaluation on bit-packed masks (cocoeval.py:164-191 computeIoU, :236-314 evaluateImg of the reference's modified
 * pycocotools; IoU semantics of maskApi.c:77-96 rleIou).  A mask of `len` elements is `stride` >= ceil(len / 64) 64-bit words, element e
 * = bit e % 64 of word e / 64, every bit past len zero.  The grouped launches read their job tables (int64, 8 entries per job) from
 * DEVICE memory; a job whose offsets do not fit the stated buffer lengths is skipped.  All results are integers or one IEEE float64
 * division of integers: nothing depends on the order of execution.
 * rsis_mask_pack_bits: masks[n][len] uint8 (zero / non-zero; the layout rsis_mask_resize_threshold writes) -> bits[n][stride],
 *   area[n] = set elements.
 * rsis_rle_to_bits: n masks from run counts (rsis_rle_encode's, or rsis_rle_from_string's): desc[k] = {first count, number of counts,
 *   first word, words} indexes counts[counts_len] / bits[bits_len]; ends[counts_len] is workspace.  sum(counts of k) must not exceed
 *   64 * words.
 * rsis_poly_to_bits: n masks from COCO polygon segmentations, bit for bit what maskApi.c:161-201 rleFrPoly gives for each part and
 *   :44-70 rleMerge (intersect = 0) for the parts of a record.  All tables in DEVICE memory: xy[2 * nverts] float64 (x, y) pairs,
 *   parts[p] = {first vertex, vertices}, recs[r] = {first part, parts, h, w, first word, words, 0, 0} (h * w < 2^31, words >=
 *   ceil(h * w / 64)); element x * h + y of record r is bit e % 64 of word bits[first word + e / 64].  scratch[bits_len] is workspace
 *   (distinct from bits; the call zeroes what it uses), area[r] = set elements.  A record or part whose entries do not fit the
 *   stated lengths is skipped.  Coordinates must be finite with |5 * coordinate| < 2^30 (the caller checks).  One block per record; its
 *   time grows with the number of walk points, 5 * the sum over edges of max(|dx|, |dy|), and with parts * words.
 * rsis_mask_intersect_blocks / _batch: jobs[j] = {dt_off, gt_off, D, G, stride, out_off, block_begin, 0}: D detection and G ground-truth
 *   masks of `stride` words (even, as are the offsets: 16-byte cells) at bits + dt_off / gt_off; inter[out_off + d * G + g] = number of
 *   elements set in both.  Job j owns blocks [block_begin_j, block_begin_j + rsis_mask_intersect_blocks(D, G, stride)); inter[inter_len]
 *   is zeroed by the call.
 * rsis_coco_iou_batch: cells[c] = {dt_begin, D, gt_begin, G, inter_off, inter_ld, iou_off, 0}:
 *   ious[iou_off + d * G + g] = i / (gt_crowd ? dt_marea : dt_marea + gt_marea - i), 0 for i = 0, with
 *   i = inter[inter_off + dt_row[dt_begin + d] * inter_ld + gt_col[gt_begin + g]].
 * rsis_coco_match_batch: cells[c] = {iou_off, D, G, dt_begin, gt_begin, dt_out, gt_out, area range}: greedy matching of D detections (in
 *   score order) against G ground truths in ignored-last order (gperm[gt_begin + g] = column of the IoU matrix, gflag = ignore |
 *   iscrowd << 1), for T <= 64 thresholds thrs[T]: dtm / dti[(dt_out + d) * T + t] = position of the matched ground truth + 1 (0: none) /
 *   ignore flag (an unmatched detection: dt_area outside arng[range]), gtm[(gt_out + g) * T + t] = position of the detection + 1.
 * rsis_rle_from_string: HOST function, inverse of rsis_rle_to_string: returns the number of counts, negated when cap is too small. */
int rsis_mask_pack_bits(const unsigned char* masks, int n, long len, unsigned long long* bits, long stride, unsigned int* area, void* stream);
int rsis_rle_to_bits(const unsigned int* counts, long counts_len, const long long* desc, int n, unsigned int* ends, unsigned long long* bits,
                     long bits_len, unsigned int* area, void* stream);
int rsis_poly_to_bits(const double* xy, long nverts, const long long* parts, long nparts, const long long* recs, int n,
                      unsigned long long* scratch, unsigned long long* bits, long bits_len, unsigned int* area, void* stream);
/* ---- COCO label maps of a whole batch, painted from the bit rows of its records at the data layer's output size (dataloader/coco.py;
 * cocomaps.hip).  bits[bits_len] / area[nrec] are what rsis_poly_to_bits / rsis_rle_to_bits left: element x * h + y of record r is bit
 * e % 64 of word bits[first word + e / 64].  All tables in DEVICE memory: recs[r] = {first word, words, native h, native w, instance id
 * (1..255), class id, 0, 0} (int64, 8 entries, nrec records); imgs[b] = {first record, records} (int64, 2 entries) for each of the B
 * samples, a sample may have 0 records; src_y[B][Ho] and src_x[B][Wo] int32: the native row / column that output row i / column j of
 * sample b samples (the caller folds resize, flip and crop into them; the kernel does no floating-point arithmetic).
 * ins[B][Ho][Wo], seg[B][Ho][Wo] int32, EVERY element written: among the sample's records whose bit at (src_x, src_y) is set, the one
 * of the SMALLEST area[] wins, equal areas go to the LOWER record index; ins = its instance id, seg = its class id; both 0 where no
 * record covers the pixel or an index lies outside [0, h) x [0, w).  A record of area 0 never wins.  A record whose entries do not
 * fit bits_len (or whose id is outside 1..255) is skipped; an image entry that does not fit nrec, or has more than max_recs records,
 * counts as 0 records.  max_recs is the caller's bound on the records of a sample: the table itself cannot be read without a copy.
 * No allocation, no host sync, no atomics, capture-safe; integer compares only, so the result does not depend on the order of
 * execution.  nrec == 0: bits / area / recs may be null.
 * RSIS_ERR_ARG, nothing launched: any other null pointer, ins == seg, an output that is also an input, B, Ho or Wo < 1, a negative
 * length.  RSIS_ERR_UNSUPPORTED, nothing launched: Ho * Wo >= 2^31, B > 65535, max_recs > 255. ---- */
int rsis_paint_instance_maps(const unsigned long long* bits, long bits_len, const unsigned int* area, long nrec, const long long* recs,
                             const long long* imgs, int B, int max_recs, const int* src_y, const int* src_x, int Ho, int Wo, int* ins, int* seg,
                             void* stream);
/* rsis_paint_ignore_map: the ignore map of the same batch (--ignore_regions).  bits[bits_len]: the bit rows of the batch's CROWD records
 * (rsis_rle_to_bits / rsis_poly_to_bits), crecs[r] = {first word, words, native h, native w, 0, 0, 0, 0} (int64, 8 entries, nrec records),
 * imgs[b] = {first crowd record, crowd records}, src_y / src_x the tables of rsis_paint_instance_maps, ins[B][Ho][Wo] the instance map it
 * painted.  ignore[B][Ho][Wo] uint8, EVERY element written: 1 where any crowd record covers (src_x, src_y) and ins is 0 there (an
 * outlined instance inside a crowd still counts), else 0.  A record that does not fit bits_len covers nothing; an image entry that does
 * not fit nrec or has more than max_recs records counts as 0 records.  No allocation, no sync, no atomics; integer compares only.
 * Same refusals as rsis_paint_instance_maps (ins == ignore or an output that is also an input: RSIS_ERR_ARG). */
int rsis_paint_ignore_map(const unsigned long long* bits, long bits_len, long nrec, const long long* crecs, const long long* imgs, int B,
                          int max_recs, const int* src_y, const int* src_x, int Ho, int Wo, const int* ins, unsigned char* ignore, void* stream);
long rsis_mask_intersect_blocks(long D, long G, long stride);
int rsis_mask_intersect_batch(const unsigned long long* bits, long bits_len, const long long* jobs, int njobs, int total_blocks,
                              unsigned int* inter, long inter_len, void* stream);
int rsis_coco_iou_batch(const long long* cells, int ncells, const unsigned int* inter, long inter_len, const int* dt_row,
                        const unsigned int* dt_marea, long ndt, const int* gt_col, const unsigned int* gt_marea, const int* gt_crowd, long ngt,
                        double* ious, long ious_len, void* stream);
int rsis_coco_match_batch(const long long* cells, int ncells, const double* ious, long ious_len, const int* gperm, const int* gflag, long ngt,
                          const double* dt_area, long ndt, const double* arng, int nrng, const double* thrs, int T, int* dtm, int* dti,
                          long dt_out_len, int* gtm, long gt_out_len, void* stream);
int rsis_rle_from_string(const char* s, unsigned int* counts, int cap);

/* ---- CVPPP leaf segmentation measures of N pairs of 8-bit label images (result `in`, ground truth `gt`, equal pixel counts per pair;
 * the challenge's Matlab scripts, reference src/CVPPP/, restated; rsis_amd/cvppp_eval.py states the definitions).  The images of a call
 * lie in ONE byte pool (16-byte aligned base; a pair may start at any offset).  Both launches read the same job table from DEVICE
 * memory, int64, 8 entries per pair: jobs[p] = {in_off, gt_off, npix, table_off, block_begin, 0, 0, 0}: the images are pool + in_off /
 * gt_off, npix bytes each (1 <= npix < 2^32); the pair's table is counts + table_off (a multiple of 4), 65536 uint32 that no other pair
 * shares; pair p owns blocks [block_begin_p, block_begin_p + rsis_label_contingency_blocks(npix_p)) of the contingency launch,
 * total_blocks = their sum.  A pair whose offsets do not fit pool_len / counts_len is skipped by both launches (its table and its
 * scores stay zero).  All results are integers or float64 operations on integers in a fixed order: they do not depend on the schedule
 * and are the same bits from run to run.
 * rsis_label_contingency_batch: counts[table_off + i * 256 + j] = number of pixels with in == i and gt == j (the marginals follow from
 *   them); counts[counts_len] is zeroed by the call.  Every pixel is read once; counts are merged in registers and in a block-private
 *   64 x 64 LDS window (labels 0 .. 63) before one integer atomic per non-zero cell and block, labels outside the window add per run.
 * rsis_label_scores_batch: scores[p][6] (zeroed by the call) = {SymmetricBestDice, FgBgDice, AbsDiffFGLabels, DiffFGLabels,
 *   BestDice(in, gt), BestDice(gt, in)} with n_i / m_j the marginals, lo / hi the smallest / largest value present in an image,
 *   Dice(i, j) = 2 o_ij / (n_i + m_j) (0 / 0 counts as 0), BestDice(in, gt) = sum over EVERY i in lo_in .. hi_in, ascending, of
 *   max_{j in lo_gt .. hi_gt} Dice(i, j), divided by hi_in - lo_in + 1; SymmetricBestDice the smaller of the two; FgBgDice =
 *   2 |F_in and F_gt| / (|F_in| + |F_gt|), F_a = {a > lo_a}, NaN when both images are constant; DiffFGLabels = (hi_in - lo_in) -
 *   (hi_gt - lo_gt). */
long rsis_label_contingency_blocks(long npix);
int rsis_label_contingency_batch(const unsigned char* pool, long pool_len, const long long* jobs, int njobs, int total_blocks,
                                 unsigned int* counts, long counts_len, void* stream);
int rsis_label_scores_batch(const unsigned int* counts, long counts_len, const long long* jobs, int njobs, double* scores, void* stream);

/* ---- Cityscapes instance-level evaluation: joint pixel counts of P binary masks against one 16-bit instance-id image, for all images of
 * a call (rsis_amd/cityscapes_eval.py states the measure; matching and AP are host float64).  The id images lie in ONE pool (16-byte
 * aligned base, pool_len BYTES, a multiple of 16; an image may start at any even byte).  Both launches read one job table from DEVICE
 * memory, int64, 16 entries per image: jobs[j] = {gt_off (bytes), npix, lut_off, bits_off, stride, P, S, counts_off, block_begin,
 * presence_block_begin, 0 ..}: 1 <= npix < 2^32 ids at pool + gt_off; flags + lut_off / lut + lut_off are the image's 65536 presence
 * bytes / id -> slot entries; its P >= 0 masks are bits + bits_off + p * stride (64-bit words, stride >= ceil(npix / 64), the layout of
 * rsis_mask_pack_bits; bits may be NULL with bits_len 0 when no image has a mask); its table is counts + counts_off, (P + 1) * S uint32
 * that no other image shares, 1 <= S <= 65535.  Image j owns blocks [block_begin_j, block_begin_j + rsis_inst_overlap_blocks(npix_j,
 * P_j)) of the overlap launch and [presence_block_begin_j, + rsis_inst_overlap_blocks(npix_j, 0)) of the presence launch; total_blocks
 * = their sum.  An image whose entries do not fit the stated buffer lengths is skipped (its flags / table stay zero).  Integer atomics
 * only: the results do not depend on the schedule.
 * rsis_inst_presence_batch: flags[lut_off + v] = 1 for every value v that occurs in the image; flags[flags_len] is zeroed by the call.
 * rsis_inst_overlap_batch: counts[counts_off + p * S + s] = #{i : bit i of mask p set and lut[gt[i]] == s} for p < P, and row p = P the
 *   histogram #{i : lut[gt[i]] == s}; a pixel whose lut entry is >= S is not counted; counts[counts_len] is zeroed by the call.  gt is
 *   read once per group of 64 masks; counts are merged in registers and in a block-private LDS window (64 masks + histogram) x 64 slots
 *   before one atomic per non-zero cell and block, slots outside the window add per run. */
long rsis_inst_overlap_blocks(long npix, long P);
int rsis_inst_presence_batch(const void* pool, long pool_len, const long long* jobs, int njobs, int total_blocks, unsigned char* flags,
                             long flags_len, void* stream);
int rsis_inst_overlap_batch(const void* pool, long pool_len, const long long* jobs, int njobs, int total_blocks, const unsigned short* lut,
                            long lut_len, const unsigned long long* bits, long bits_len, unsigned int* counts, long counts_len, void* stream);

/* ---- channel-blocked bf16 activations: the storage half of the bf16 path (BASELINE.json configs[2..4]) --------------------------
 * A logical [B][C][H][W] tensor stored as bf16 [B][C/8][H][W][8] ("blk": the 8 channels of a pixel are one 16-byte cell, C % 8 == 0).
 * The reference has no counterpart (fp32 NCHW throughout); these entry points serve the ResNet-101 trunk of
 * src/modules/vision.py:12-19 under -dtype bf16. */

/* fp32 NCHW -> blk (round-to-nearest-even) and back (exact) */
int rsis_blk_from_nchw(const float* x, void* y_blk, int B, int C, int H, int W, void* stream);
int rsis_blk_to_nchw(const void* x_blk, float* y, int B, int C, int H, int W, void* stream);

/* out_blk[B][Cout] = conv(x_blk[B][C], W), ks in {1, 3}, stride 1, "same" padding, no bias (torchvision's trunk convs have none);
 * Wp: the bf16 pack rsis_conv_pack_fwd (forward) or rsis_conv_pack_dgrad (data gradient: x = dy, out = dx) produce for dtype
 * RSIS_DTYPE_BF16.  addend_blk (optional, the output's shape; may alias out_blk) is added in fp32 before the ONE rounding to bf16 at
 * the store.  variant: 0 = pick a tile, > 0 force (tests).  C and Cout need only be multiples of 8: the ring stages hold 16 (3x3) or 32
 * (1x1) input channels, and a ragged last stage reads zero cells (descriptor range) against the pack's zero-padded rows. */
int rsis_blk_conv2d(const void* x_blk, int B, int C, int H, int W, const void* Wp, int Cout, int ks, const void* addend_blk,
                    void* out_blk, int variant, void* stream);
/* ... followed by the eval-mode BatchNorm of its output IN THE EPILOGUE (inference: test(), reference src/test.py:35-38; every trunk
 * conv is followed by one): out = relu?(v * sc + sh (+ addend)), sc = gamma * rsqrt(running_var + eps), sh = beta - running_mean * sc, where
 * v is the product rounded to bf16 (single_rounding = 0: bit for bit what rsis_blk_conv2d + rsis_blk_bn_fwd (eval) compute, without the
 * BatchNorm launch) or kept in fp32 (single_rounding = 1: closer to the fp32 result).  gamma .. running_var: fp32 [Cout]. */
int rsis_blk_conv2d_bn_eval(const void* x_blk, int B, int C, int H, int W, const void* Wp, int Cout, int ks, const void* addend_blk,
                            const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, int relu,
                            int single_rounding, void* out_blk, int variant, void* stream);

/* BatchNorm2d (+ residual add) (+ ReLU) on blk tensors: y = relu?((x - mean) * rstd * gamma + beta (+ res)).  train != 0: batch
 * statistics (saved to save_mean / save_rstd for the backward; run_mean / run_var, if given, updated with `momentum` and the unbiased
 * variance, as nn.BatchNorm2d does); train == 0: normalises with run_mean / run_var.  scratch: rsis_blk_bn_scratch_doubles(C) doubles
 * (per-split partial sums: the reduction order is fixed, results are bit-reproducible). */
long rsis_blk_bn_scratch_doubles(int C);
int rsis_blk_bn_fwd(const void* x_blk, const void* res_blk, void* y_blk, double* scratch, const float* gamma, const float* beta,
                    float* run_mean, float* run_var, float* save_mean, float* save_rstd, int B, int C, int H, int W, float eps,
                    float momentum, int relu, int train, void* stream);
/* backward of the train-mode forward: g = dy * [y > 0] if relu (y_blk = the forward output; NULL: the mask is recomputed from x -- only
 * valid without a residual), dx = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)), dres_blk (optional) = g, the gradient of the
 * residual branch; dgamma / dbeta (optional) = sum g * xhat / sum g, added to the buffers if accumulate != 0, stored otherwise. */
int rsis_blk_bn_bwd(const void* dy_blk, const void* x_blk, const void* y_blk, double* scratch, const float* gamma, const float* beta,
                    const float* save_mean, const float* save_rstd, void* dx_blk, void* dres_blk, float* dgamma, float* dbeta,
                    int accumulate, int B, int C, int H, int W, int relu, void* stream);
/* y[oh][ow] = x[oh * stride][ow * stride] (a strided conv = the stride-1 conv, then this) and its transpose (dx of H x W: dy at the
 * multiples of stride, zero elsewhere) */
int rsis_blk_subsample2d(const void* x_blk, void* y_blk, int B, int C, int H, int W, int stride, void* stream);
int rsis_blk_upscatter2d(const void* dy_blk, void* dx_blk, int B, int C, int H, int W, int stride, void* stream);

/* ---- the recurrent decoder on blk tensors (ConvLSTM cells of clstm.py:19-62 inside the loop of model.py:129-165, run over the
 * (level, timestep) wavefront: the cells of a diagonal are independent, so every entry point below takes SEVERAL independent jobs
 * and runs them in one grid where it can).  Reference arithmetic with bf16 operands / storage: fp32 accumulation and cell update,
 * ONE rounding at each blk store; the cell state c stays fp32 NCHW. ---- */

/* One 3x3 / stride 1 / pad 1 conv over the channel concat of nsrc <= 3 blk sources.  Wp: the RSIS_DTYPE_BF16 pack of
 * rsis_conv_pack_fwd (or _dgrad: the job is then the data gradient, sources = dy) built for the same segments; Cpack = the pack's
 * row count (Cout of rsis_conv_pack_fwd, Cin_packed of rsis_conv_pack_dgrad; 0 = Cout).
 *   hid == 0, plain epilogue: out = conv (+ bias[Cout], fp32, packed row order) (+ addend, blk [B][Cout]) split over ndst <= 2 blk
 *     destinations of Cdst[i] channels (Cdst % 8 == 0, sum = Cout <= Cpack: leading rows of the pack);
 *   hid > 0, fused ConvLSTM cell (rows gate-interleaved 4 j + gate, Cout = 4 hid, hid % 8 == 0): gates = conv (+ bias) + addend (blk
 *     [B][4 hid], the time-invariant skip term) -> i, f, o = sigmoid, g = tanh, c = f c_prev + i g, h = o tanh(c).  c_prev (NULL = zero
 *     state) / c_out: fp32 [B][hid][H][W]; h_out: blk [B][hid]; act_out (may be NULL): blk [B][4 hid], the post-nonlinearity gates;
 *     side_key (may be NULL): [B][hid] keys of the global max-pool of h (fp32, before the rounding of h_out), as rsis_lstm_job.side_key.  nsrc may be 0. */
typedef struct rsis_blk_conv_job {
  const void* src[3];
  int Csrc[3];
  int nsrc, B, H, W;
  const void* Wp;
  int Cout, Cpack;
  const float* bias;
  const void* addend;
  void* dst[2];
  int Cdst[2];
  int ndst;
  int hid;
  const float* c_prev;
  float* c_out;
  void* h_out;
  void* act_out;
  unsigned long long* side_key;
  int tile;              /* 0 = the library picks the MFMA tile; 1 / 4 / 5 force one (tests) */
} rsis_blk_conv_job;
int rsis_blk_conv3x3_batch(const rsis_blk_conv_job* jobs, int njobs, void* stream);

/* align-corners bilinear resize (nn.UpsamplingBilinear2d, model.py:149-150,163-164) of blk tensors, x [B][C][Hi][Wi] -> y [B][C][Ho][Wo],
 * and its transpose dx = resize^T(dy); with dpool / arg (both [B][C], or both NULL) the transpose also adds dpool[b][c] at flat pixel
 * arg[b][c] of every channel plane: the gradient of the global max-pool side feature (model.py:143) of the same tensor. */
typedef struct rsis_blk_resize_job {
  const void* src;       /* forward: x; backward: dy */
  void* dst;             /* forward: y; backward: dx */
  const float* dpool;
  const int* arg;
  int B, C, Hi, Wi, Ho, Wo;
} rsis_blk_resize_job;
int rsis_blk_upsample_fwd_batch(const rsis_blk_resize_job* jobs, int njobs, void* stream);
int rsis_blk_upsample_bwd_batch(const rsis_blk_resize_job* jobs, int njobs, void* stream);
/* The same two with the decoder's Dropout2d scale: channel plane (b, c) of the result (forward: y; backward: dx, after dpool was added) is
 * multiplied by scale[b][c] ([B][C] fp32; NULL = the unscaled job) in fp32 before the one rounding to bf16. */
typedef struct rsis_blk_resize_scaled_job {
  const void* src;
  void* dst;
  const float* dpool;
  const int* arg;
  int B, C, Hi, Wi, Ho, Wo;
  const float* scale;
} rsis_blk_resize_scaled_job;
int rsis_blk_upsample_fwd_scaled_batch(const rsis_blk_resize_scaled_job* jobs, int njobs, void* stream);
int rsis_blk_upsample_bwd_scaled_batch(const rsis_blk_resize_scaled_job* jobs, int njobs, void* stream);

/* `-skip_mode mul` on blk tensors.  Forward: y = resize(x) * mul, mul a blk tensor of y's shape; blend and product in fp32, ONE rounding
 * to bf16 at the store. */
typedef struct rsis_blk_resize_mul_job {
  const void* src;
  void* dst;
  int B, C, Hi, Wi, Ho, Wo;
  const void* mul;
} rsis_blk_resize_mul_job;
int rsis_blk_upsample_mul_fwd_batch(const rsis_blk_resize_mul_job* jobs, int njobs, void* stream);
/* Backward preparation at the fine resolution, in front of rsis_blk_upsample_bwd_batch.  With u = resize(x) as rsis_blk_upsample_fwd_batch
 * stores it (rounded to bf16):  dm = accumulate ? fmaf(dy, u, dm) : dy * u  into the fp32 NCHW accumulator dm [B][C][Ho][Wo] (the caller
 * rounds it to bf16 once, after the last step), then dy <- dy * m in place with one rounding. */
typedef struct rsis_blk_mul_prep_job {
  void* dy;              /* blk [B][C][Ho][Wo], read and overwritten */
  const void* x;         /* blk [B][C][Hi][Wi] */
  const void* m;         /* blk [B][C][Ho][Wo] */
  float* dm;
  int B, C, Hi, Wi, Ho, Wo;
  int accumulate;        /* 0 = store, 1 = add */
} rsis_blk_mul_prep_job;
int rsis_blk_upsample_mul_bwd_prep_batch(const rsis_blk_mul_prep_job* jobs, int njobs, void* stream);

/* rsis_convlstm_bwd_gates on blk tensors: dh, dh2 (may be NULL) blk [B][hid]; act, da blk [B][4 hid] (rows 4 j + gate); c, c_prev,
 * dc_next, dc_prev fp32 [B][hid][HW] (c_prev / dc_next / dc_prev may be NULL). */
typedef struct rsis_blk_lstm_bwd_job {
  const void* dh;
  const void* dh2;
  const float* dc_next;
  const void* act;
  const float* c_prev;
  const float* c;
  void* da;
  float* dc_prev;
  int B, hid, HW;
} rsis_blk_lstm_bwd_job;
int rsis_blk_lstm_bwd_batch(const rsis_blk_lstm_bwd_job* jobs, int njobs, void* stream);

/* y_blk[cell] = sum_t x_blk[t][cell] over T stacked blk tensors of ncells 16-byte cells each (fp32 accumulation, t ascending, one
 * rounding): the sum over the timesteps of d(gates), i.e. the gradient of a level's time-invariant gate term */
int rsis_blk_sum_leading(const void* x_blk, void* y_blk, int T, long ncells, void* stream);
/* rsis_bias_grad for a blk dy [B][C][HW]: db[C] += sum over (b, pixel); lstm_hid > 0: blk channel 4 j + gate -> db[gate * hid + j] */
int rsis_blk_bias_grad(const void* dy_blk, float* db, int B, int C, int HW, int lstm_hid, void* stream);

/* conv_out (model.py:109,167; Cin == 8: hidden_size / 16 at hidden_size 128) over all T timesteps from the blk hidden state:
 * x / dx blk [T][B][8][H][W]; y / dy fp32 [B][T][H*W]; Wref = the reference-layout weight [1][8][3][3] (fp32, no pack); bias [1] or
 * NULL; dW[72] / db[1] (db may be NULL) are ACCUMULATED.  W % 4 == 0. */
int rsis_blk_conv_out_seq_fwd(const void* x, const float* Wref, const float* bias, float* y, int T, int B, int H, int W, void* stream);
int rsis_blk_conv_out_seq_dgrad(const float* dy, const float* Wref, void* dx, int T, int B, int H, int W, void* stream);
int rsis_blk_conv_out_seq_wgrad(const float* dy, const void* x, float* dW, float* db, int T, int B, int H, int W, void* stream);

/* The decoder's tail as one op per direction (upconv_out.hip): nn.UpsamplingBilinear2d (align_corners, model.py:163-164) of the last
 * level's hidden state followed by conv_out (model.py:109,167: Conv2d(8 -> 1, 3x3, pad 1)) over the images of all T timesteps, without
 * forming the upsampled tensor.  h / dh: fp32 [T][B][8][Hs][Ws] (h_blk = 0) or bf16 blk [T][B][1][Hs][Ws][8] (h_blk = 1); out / dout:
 * fp32 [B][T][Ho*Wo]; w = the reference-layout weight [1][8][3][3]; bias [1] or NULL.  Backward: dh is WRITTEN (plus, when dside /
 * arg are given, the gradient dside[T*B][8] of the side max-pool feature at its arg-max pixel arg[T*B][8], model.py:143); dW[72] and
 * db[1] (either may be NULL) are ACCUMULATED, from per-block sums in `partial` (rsis_upconv_out_bwd_blocks(..) x 80 floats of
 * scratch) added in a fixed order: reproducible run to run.  rsis_upconv_out_supported: C == 8 and an upsampling factor of ~2
 * (scale (in-1)/(out-1) in [0.46, 0.52]); otherwise RSIS_ERR_UNSUPPORTED (run rsis_upsample_* + rsis_conv_out_seq_* instead). */
int rsis_upconv_out_supported(int C, int Hs, int Ws, int Ho, int Wo);
int rsis_upconv_out_bwd_blocks(int T, int B, int Hs, int Ws);
int rsis_upconv_out_fwd(const void* h, int h_blk, const float* w, const float* bias, float* out, int T, int B, int C, int Hs, int Ws, int Ho, int Wo,
                        void* stream);
int rsis_upconv_out_bwd(const float* dout, const void* h, int h_blk, const float* w, void* dh, float* dW, float* db, const float* dside, const int* arg,
                        float* partial, int T, int B, int C, int Hs, int Ws, int Ho, int Wo, void* stream);

/* ---- gradient exchange: RCCL bound directly (replaces nn.DataParallel, reference src/train.py:269-274: one process per GPU, the flat
 * gradient buffers SUM-all-reduced over xGMI once per iteration).  A collective issued here is an ordinary operation of `stream`: it
 * can be captured into the hipGraph of the training iteration (torch.distributed's ProcessGroupNCCL cannot: its watchdog thread's
 * event queries abort a concurrent stream capture).  RCCL is resolved at run time (dlopen); RSIS_ERR_UNSUPPORTED if it is not there.
 *   rsis_comm_available : RSIS_OK iff librccl resolves in this process (dlopen + symbols only: no bootstrap listener, no device work);
 *                         what every rank calls to AGREE on the direct exchange before anything that can block inside RCCL;
 *   rsis_comm_unique_id : rank 0 fills id_out[128] (ncclUniqueId); the caller distributes it to the other ranks (any channel);
 *   rsis_comm_init      : collective over the `world` ranks, each on its own current HIP device; *comm receives the communicator;
 *   rsis_comm_size      : number of ranks of the communicator (-1 on error);
 *   rsis_comm_allreduce_sum_f32 : buf[n] <- sum over ranks, in place, enqueued on `stream`;
 *   rsis_comm_destroy, rsis_comm_last_error (text of the last RCCL failure of this process). ---- */
int rsis_comm_available(void);
int rsis_comm_unique_id(void* id_out);
int rsis_comm_init(void** comm, int world, int rank, const void* id);
int rsis_comm_size(void* comm);
int rsis_comm_allreduce_sum_f32(void* comm, float* buf, long n, void* stream);
int rsis_comm_destroy(void* comm);
const char* rsis_comm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RSIS_HIP_H */
