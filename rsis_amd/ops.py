"""torch.autograd.Function wrappers over the C ABI of librsis_hip.so (include/rsis_hip.h).

PyTorch is plumbing here (device memory, streams, the autograd tape); every arithmetic op of the hot path runs in
the hand-written gfx950 kernels.  There is no CPU/eager fallback: the ops raise if the library is missing or a
tensor is not a CUDA fp32 tensor.
"""
import ctypes
import os
import weakref

import torch

from . import _lib
from ._lib import check, int_array, lib, ptr, ptr_array, require_cuda_f32, stream

# Bumped whenever parameters are modified behind autograd's back (the flat HIP Adam step, load_state_dict):
# invalidates every packed-weight cache.
_WEIGHT_EPOCH = [0]


# Test hook: force the MFMA tile configuration of the implicit-GEMM kernels (0 = library heuristic).
FORCE_TILE = [0]


# Accumulate weight / bias / BN-affine gradients straight into a pre-zeroed, contiguous `param.grad` (the flat gradient
# buffer of rsis_amd.optim.FlatGroup) instead of materialising a zero-filled tensor per parameter and letting autograd add
# it: ~3 small launches less per parameter per step.  Off by default (plain autograd semantics); the training driver turns it
# on.  Autograd still runs the parameter's AccumulateGrad node (with an undefined gradient), so post-accumulate hooks --
# the bucketed all-reduce -- keep firing in the right order.
DIRECT_GRAD = [False]


def _direct_target(param):
    g = param.grad if DIRECT_GRAD[0] and param is not None else None
    return g if (g is not None and g.is_contiguous() and g.dtype == torch.float32 and g.is_cuda) else None


# arithmetic of the MFMA conv kernels (include/rsis_hip.h RSIS_DTYPE_*); a property of each PackedConv, set from `-dtype`
DTYPE_F32, DTYPE_BF16 = 0, 1
DTYPE_F32_WINO = 3      # include/rsis_hip.h RSIS_DTYPE_F32_WINO: exact-f32 arithmetic, eligible 3x3 convs as Winograd F(2x2, 3x3)
DTYPE_F32_LIMB = 4      # include/rsis_hip.h RSIS_DTYPE_F32_LIMB: fp32 operands as three bf16 limbs each, training calls of eligible 3x3 convs


def _wino_rule():
    """RSIS_WINOGRAD: which fp32 3x3 / stride 1 / pad 1 convs run as Winograd F(2x2, 3x3) on the f32 MFMA (conv_wino.hip).
    "0" = none; "all" = every conv the kernel covers (rsis_conv_uses_wino); a comma list of channel counts = the square convs
    (Cin == Cout) of those widths.  Default "64,128,256": the stride-1 bottleneck convs of ResNet-101 layers 1-3 (3 + 3 + 22 convs; per shape,
    tools/wino_bench.py: 256 @16^2 90 -> 56 us, 128 @32^2 78 -> 56, 64 @64^2 75 -> 68; NOT layer 4: 512 @8^2 fills a quarter of the
    64-tile block, 98 -> 176 us)."""
    v = os.environ.get("RSIS_WINOGRAD", "64,128,256").strip().lower()
    if v in ("0", "", "off", "none"):
        return None
    if v == "all":
        return "all"
    return {int(t) for t in v.split(",") if t.strip()}


WINOGRAD = [_wino_rule()]

# the classes of the fp32 step whose training-call 3x3 convs run the limb flavour of the direct kernel (csrc/conv3x3_limb.h,
# DTYPE_F32_LIMB).  A class is a decoder level, forward and gradient separately: "f<i>" = the gate forward of ConvLSTM level i (i = 0 the
# coarsest map), "d<i>" = its gate data gradient where the Winograd rule does not take it.  RSIS_CONV_LIMBS: "0" = none (every conv on the
# f32 MFMA, the routing before the limb kernel existed), "all" = every class, or a comma list of classes.  The default is what measured
# faster inside a replayed 256 x 256 / T = 10 / B = 32 step (NOTES.md (95)).
LIMB_DEFAULT = "f1,f2,f3,f4,d3,d4"


def _limb_rule():
    v = os.environ.get("RSIS_CONV_LIMBS", LIMB_DEFAULT).strip().lower()
    if v in ("0", "", "off", "none"):
        return frozenset()
    if v == "all":
        return "all"
    return frozenset(t.strip() for t in v.split(",") if t.strip())


LIMBS = [_limb_rule()]


def limb_class(name):
    """does the routing put class `name` ("f2", "d4", ...) on the limb kernel?"""
    rule = LIMBS[0]
    return rule == "all" or name in rule
# Winograd also on the inference / parity path (no_grad calls: test(), eval.py)?  Default off: those calls keep the direct kernel with
# segmented accumulation, bit for bit what they computed before the Winograd kernel existed.  Measured with it on (round 6): every
# e2e golden still within 1e-4 of the reference, but on the HOT fixture (e2e_256_hot: |logit| to 5.5, half the gates saturated) the
# worst mask logit moves from 1.08e-4 to 1.86e-4 from float64 (the reference itself: 1.0e-4) -- 22 stacked Winograd layers are as
# accurate per layer as an unsegmented direct sum (2.8e-6 vs 2.6e-6 on O(1) data), not as accurate as the segmented one.
# set by FeatureExtractor.forward around a TRAINING forward that runs under no_grad (the frozen trunk: modules/model.py trunk_grad): the
# convs then take the kernels of a training call (Winograd where the rule says so, split-K allowed) -- the same arithmetic as the
# iteration that does back-propagate through them -- instead of the inference / parity instantiations
TRAINING_FORWARD = [False]
WINOGRAD_INFER = [os.environ.get("RSIS_WINOGRAD_INFER", "0") == "1"]
# the decoder's gate data gradients (training only) on the Winograd kernel where the level qualifies (decoder_fused.dyn_dgrad_pack)
WINOGRAD_GATES = [os.environ.get("RSIS_WINOGRAD_GATES", "1") != "0" and os.environ.get("RSIS_WINOGRAD", "x").strip().lower() not in ("0", "off", "none")]


def conv_dtype(dtype, ks, stride, pad, cin, cout):
    """the dtype a plain conv's PackedConv is built with: fp32 convs the Winograd rule selects get DTYPE_F32_WINO"""
    d = int(dtype)
    rule = WINOGRAD[0]
    if d != DTYPE_F32 or rule is None or not lib().rsis_conv_uses_wino(int(ks), int(stride), int(pad), int(cin), int(cout), 1, 0):
        return d
    return DTYPE_F32_WINO if (rule == "all" or (cin == cout and cin in rule)) else d

DTYPES = {"fp32": DTYPE_F32, "f32": DTYPE_F32, "float32": DTYPE_F32, "bf16": DTYPE_BF16, "bfloat16": DTYPE_BF16}


def set_dtype(module, dtype):
    """Switch every conv / ConvLSTM of a module tree to the f32 or bf16 MFMA kernels (parameters stay fp32)."""
    d = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    for m in module.modules():
        if hasattr(m, "_set_rsis_dtype"):
            m._set_rsis_dtype(d)
    return module


def set_deterministic(on=True):
    """Bit-reproducible mode of the library (include/rsis_hip.h: rsis_set_deterministic): every reduction gets a single
    contributor per address, so two runs -- or an eager run and a hipGraph replay -- produce identical bits.  Slower (launches
    stop filling the chip); returns the previous setting.  RSIS_DETERMINISTIC=1 turns it on from the environment."""
    return bool(lib().rsis_set_deterministic(1 if on else 0))


def is_deterministic():
    return bool(lib().rsis_get_deterministic())


SUBSAMPLE_1X1 = [os.environ.get("RSIS_SUBSAMPLE_1X1", "1") != "0"]     # A/B switch, see _Conv2dFn.forward
_PACKS = weakref.WeakSet()       # every PackedConv that holds a packed copy
_BATCH = {"sig": None, "jobs": None, "n": 0, "blocks": 0}


def repack_all():
    """Rebuild every packed weight copy in ONE launch (rsis_conv_pack_batch) -- call after the optimizer step.  Without it
    each PackedConv repacks lazily at its next use: ~240 launches of ~5 us per training step."""
    L = lib()
    todo = []
    for p in list(_PACKS):
        w = p._refs[0]() if p._refs is not None else None
        if w is None or not w.is_cuda:
            continue
        b = p._refs[1]() if p._refs[1] is not None else None
        if p.wp is not None and p._key_f is not None:
            todo.append((p, w, b, p.wp, 0))
        if p.wd is not None and p._key_d is not None:
            todo.append((p, w, b, p.wd, 1))
    if not todo:
        return
    sig = tuple(p._job_sig(w, out, d) for p, w, _b, out, d in todo)
    if _BATCH["sig"] != sig:                       # (re)build the device-side job table: pointers are stable across steps
        jobs = (_lib.PackJob * len(todo))()
        blocks = 0
        for i, (p, w, _b, out, d) in enumerate(todo):
            jobs[i] = p._job(w, out, d)
            nb = L.rsis_conv_pack_job_fill(ctypes.byref(jobs[i]))
            if nb < 0:
                raise _lib.RsisHipError("rsis_conv_pack_job_fill rejected a pack job")
            jobs[i].block_begin = blocks
            blocks += nb
        raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(todo[0][1].device)
        _BATCH.update(sig=sig, jobs=raw, n=len(todo), blocks=blocks)
    check(L.rsis_conv_pack_batch(ptr(_BATCH["jobs"]), _BATCH["n"], _BATCH["blocks"], stream()), "rsis_conv_pack_batch")
    for p, w, b, _out, d in todo:
        if d == 0:
            p._key_f = p._key(w) + ((b._version, b.data_ptr()) if b is not None else ())
            if b is not None and p.lstm_hid > 0:
                p._pack_bias(b)
        else:
            p._key_d = p._key(w)


def bump_weight_epoch():
    _WEIGHT_EPOCH[0] += 1


class PackedConv(object):
    """Private MFMA-friendly copies of one nn.Conv2d weight (never serialised; rebuilt when the weight changes).

    segs / offs: channel counts (and offsets inside the weight's input channels; default consecutive) of the tensors the
    conv gathers from -- the channel concat (torch.cat folded into the kernel) or a subset of the input channels.
    lstm_hid > 0: ConvLSTM `Gates` conv -- rows [i|f|o|g] are interleaved to 4*j+gate (clstm.py:47).
    """

    def __init__(self, ks, segs, lstm_hid=0, stride=1, pad=None, offs=None, dtype=DTYPE_F32):
        self.dtype = int(dtype)
        if int(lstm_hid) > 0 and int(ks) != 3:
            # the fused-cell epilogue of the bf16 kernels exists for 3x3 gates only (rsis_convlstm_fwd returns UNSUPPORTED otherwise):
            # a ConvLSTM with another kernel size keeps the f32 kernels -- packing, forward, data and weight gradient alike
            self.dtype = DTYPE_F32
        self.ks = int(ks)
        self.stride = int(stride)
        self.pad = int(ks // 2 if pad is None else pad)
        self.segs = [int(s) for s in segs]
        self.offs = [int(o) for o in offs] if offs is not None else None
        self.cin = sum(self.segs)
        self.lstm_hid = int(lstm_hid)
        self._key_f = None
        self._key_d = None
        self.training_call = False
        self._twin = None
        self.wp = None
        self.wd = None
        self.bias_p = None
        self._refs = None

    def _key(self, w):
        return (_WEIGHT_EPOCH[0], w._version, w.data_ptr(), self.dtype)

    def direct_twin(self):
        """the RSIS_DTYPE_F32 copy set of a Winograd-packed conv (same geometry): what its inference / parity calls run on"""
        if self._twin is None:
            self._twin = PackedConv(self.ks, self.segs, lstm_hid=self.lstm_hid, stride=self.stride, pad=self.pad, offs=self.offs, dtype=DTYPE_F32)
        return self._twin

    def _pack_bias(self, bias):
        """gate-interleaved copy of a ConvLSTM bias (row 4*j + gate), refreshed IN PLACE in a buffer allocated once: the kernels of
        a captured training iteration read this address in its forward part and repack_all() rewrites it at the end of the same
        capture -- a freshly allocated tensor per repack would leave every replay after the first reading the capture-time values
        (in freed memory)."""
        n = 4 * self.lstm_hid
        if self.bias_p is None or self.bias_p.numel() != n or self.bias_p.device != bias.device:
            self.bias_p = torch.empty(n, dtype=torch.float32, device=bias.device)
        self.bias_p.view(self.lstm_hid, 4).copy_(bias.detach().view(4, self.lstm_hid).t())

    def _job(self, w, out, dgrad):
        j = _lib.PackJob()
        j.W, j.out, j.dgrad, j.dtype = w.data_ptr(), out.data_ptr(), int(dgrad), self.dtype
        j.Cout, j.Ctot, j.ks, j.stride, j.pad = w.shape[0], w.shape[1], self.ks, self.stride, self.pad
        j.nseg, j.lstm_hid = len(self.segs), self.lstm_hid
        off = 0
        for i, c in enumerate(self.segs):
            j.Cseg[i] = c
            j.Coff[i] = self.offs[i] if self.offs is not None else off
            off += c
        return j

    def _job_sig(self, w, out, dgrad):
        """everything _job() puts into a pack job, as a tuple: repack_all() keeps its device-side job table while these stay the same.
        (Not id(self) and the two addresses alone: a PackedConv created after another was freed can get its id AND the addresses of its
        weight and its copy from the allocator's free lists, with another geometry -- the table of the dead one then packed the new one.)"""
        return (w.data_ptr(), out.data_ptr(), int(dgrad), self.dtype, tuple(w.shape), self.ks, self.stride, self.pad, tuple(self.segs),
                tuple(self.offs) if self.offs is not None else None, self.lstm_hid)

    def _seg_args(self):
        return len(self.segs), int_array(self.segs), (int_array(self.offs) if self.offs is not None else None)

    def fwd(self, w, bias=None):
        key = self._key(w) + ((bias._version, bias.data_ptr()) if bias is not None else ())
        if self._key_f != key:
            L = lib()
            Cout, Ctot = w.shape[0], w.shape[1]
            nseg, segs, offs = self._seg_args()
            n = L.rsis_conv_packed_bytes_fwd(self.dtype, Cout, self.ks, self.stride, self.pad, nseg, segs) // 4
            if self.wp is None or self.wp.numel() != n:
                self.wp = torch.zeros(n, dtype=torch.float32, device=w.device)     # raw bytes (f32 rows or bf16 cells); may leave slack
            check(L.rsis_conv_pack_fwd(ptr(w.detach()), ptr(self.wp), Cout, Ctot, self.ks, self.stride, self.pad, nseg, segs, offs,
                                       self.lstm_hid, self.dtype, stream()), "rsis_conv_pack_fwd")
            if bias is not None and self.lstm_hid > 0:
                self._pack_bias(bias)
            self._key_f = key
            self._refs = (weakref.ref(w), weakref.ref(bias) if bias is not None else None)
            _PACKS.add(self)
        return self.wp

    def dgrad(self, w):
        key = self._key(w)
        if self._key_d != key:
            L = lib()
            Cout, Ctot = w.shape[0], w.shape[1]
            nseg, segs, offs = self._seg_args()
            n = L.rsis_conv_packed_bytes_dgrad(self.dtype, Cout, self.ks, self.stride, self.pad, self.cin) // 4
            if self.wd is None or self.wd.numel() != n:
                self.wd = torch.zeros(n, dtype=torch.float32, device=w.device)
            check(L.rsis_conv_pack_dgrad(ptr(w.detach()), ptr(self.wd), Cout, Ctot, self.ks, self.stride, self.pad, nseg, segs, offs,
                                         self.lstm_hid, self.dtype, stream()), "rsis_conv_pack_dgrad")
            self._key_d = key
            if self._refs is None:
                self._refs = (weakref.ref(w), None)
            _PACKS.add(self)
        return self.wd


def _contig(t):
    return t if t.is_contiguous() else t.contiguous()


def _conv_out_size(n, ks, stride, pad):
    return (n + 2 * pad - ks) // stride + 1


def _dgrad_all(L, dy, wd, cin_packed, ks, stride, pad, srcs, Hx, Wx, addend=None, inplace=False, dtype=DTYPE_F32):
    """One dgrad launch producing the gradient of every concat source (+ addend: another consumer's gradient of the input;
    inplace: the strided 1x1 gradient is accumulated INTO the addend tensor, which becomes the result)."""
    B, Cout, Hy, Wy = dy.shape
    # srcs: the conv's inputs, or just their shapes (the strided 1x1 path keeps a sub-sampled copy instead of the input)
    shapes = [tuple(s.shape) if torch.is_tensor(s) else tuple(s) for s in srcs]
    dxs = [addend] if inplace else [torch.empty(sh, dtype=torch.float32, device=dy.device) for sh in shapes]
    check(L.rsis_conv2d_dgrad(ptr(dy), B, Cout, Hy, Wy, ptr(wd), cin_packed, ks, stride, pad, ptr_array(dxs),
                              int_array([sh[1] for sh in shapes]), len(shapes), Hx, Wx, ptr(addend), FORCE_TILE[0], dtype, stream()),
          "rsis_conv2d_dgrad")
    return dxs


class GradSlot(object):
    """Hand-over of a gradient between two autograd nodes that consume the SAME tensor, so that the consumer's data-gradient
    kernel adds it in its epilogue instead of autograd running a full-size `add`:
      * identity residual block: the input feeds conv1 and, as the identity branch, the block's last BatchNorm; the BatchNorm
        backward parks its identity-branch gradient, conv1's dgrad takes it;
      * downsample block: the input feeds conv1 and the downsample conv; the downsample conv's dgrad (created later in the
        forward, hence run earlier by autograd) parks its result, conv1's dgrad takes it;
      * a trunk feature that also leaves the trunk (skip connection): `grad_tap` parks the outside gradient for the next
        stage's downsample conv, whose strided 1x1 dgrad accumulates into it in place.
    `park` refuses (the producer then returns its gradient the normal way) once the consumer has run, so the sum is right
    whatever order autograd picks."""

    def __init__(self):
        self.grad = None
        self.done = False

    def reset(self):
        self.grad, self.done = None, False

    def take(self):
        g, self.grad = self.grad, None
        self.done = True
        return g

    def park(self, g):
        if self.done or self.grad is not None or g is None:
            return False
        self.grad = g
        return True


class _GradTapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slot):
        ctx.slot = slot
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        if g is not None and ctx.slot.park(g if g.is_contiguous() else g.contiguous()):
            return None, None
        return g, None


def grad_tap(x, slot):
    """Identity whose backward parks the incoming gradient in `slot` (see GradSlot) instead of returning it."""
    if slot is None or not (torch.is_grad_enabled() and x.requires_grad):
        return x
    return _GradTapFn.apply(x, slot)


# Parked weight gradients.  Nothing reads a weight gradient before the optimizer step (or, one process per GPU, before its bucket is
# all-reduced), so while the training driver has DIRECT_GRAD on -- the result goes straight into the flat gradient buffer, autograd
# never sees it -- the launches are queued and flushed together through rsis_conv2d_wgrad_batch: one grid per tile configuration
# over ~40 layers instead of ~95 launches that each split their pixel axis 8-32 ways to fill the chip alone (include/rsis_hip.h).
# The queue keeps dy / x / dW alive until the flush.
WGRAD_DEFER = [False]
_WGRAD_QUEUE = []


def wgrad_launch(L, dy, x, dW, B, Cs, H, W, Cout, Ho, Wo, ks, stride, pad, Ctot, c_off, lstm_hid, dtype, what, direct):
    """rsis_conv2d_wgrad now, or parked until flush_wgrads() (only when dW is the flat-buffer target: `direct`)"""
    if direct and WGRAD_DEFER[0]:
        _WGRAD_QUEUE.append(((dy.data_ptr(), x.data_ptr(), dW.data_ptr(), B, Cs, H, W, Cout, Ho, Wo, ks, stride, pad, Ctot, c_off, lstm_hid,
                              dtype), (dy, x, dW)))
        return
    check(L.rsis_conv2d_wgrad(ptr(dy), ptr(x), ptr(dW), B, Cs, H, W, Cout, Ho, Wo, ks, stride, pad, Ctot, c_off, lstm_hid, dtype, stream()), what)


def flush_wgrads():
    """launch every parked weight gradient (call before anything reads the flat gradient buffers)"""
    n = len(_WGRAD_QUEUE)
    if n == 0:
        return
    jobs = (_lib.WgradJob * n)()
    for j, (f, _keep) in zip(jobs, _WGRAD_QUEUE):
        (j.dy, j.x, j.dW, j.B, j.Cs, j.H, j.W, j.Cout, j.Ho, j.Wo, j.ks, j.stride, j.pad, j.Ctot, j.c_off, j.lstm_hid, j.dtype) = f
    try:
        check(lib().rsis_conv2d_wgrad_batch(jobs, n, stream()), "rsis_conv2d_wgrad_batch")
    finally:
        del _WGRAD_QUEUE[:]


def _wgrad_all(L, dy, srcs, w_shape, ks, stride, pad, lstm_hid, out=None, dtype=DTYPE_F32):
    B, Cout, Ho, Wo = dy.shape
    Ctot = w_shape[1]
    dW = out if out is not None else torch.zeros(w_shape, dtype=torch.float32, device=dy.device)
    c_off = 0
    for s in srcs:
        _, Cs, H, W = s.shape
        wgrad_launch(L, dy, s, dW, B, Cs, H, W, Cout, Ho, Wo, ks, stride, pad, Ctot, c_off, lstm_hid, dtype, "rsis_conv2d_wgrad",
                     out is not None)
        c_off += Cs
    return dW


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pack, stride, pad, nsrc, slot, *tensors):
        srcs = [_contig(t) for t in tensors[:nsrc]]
        weight, bias = tensors[nsrc], tensors[nsrc + 1]
        ctx.slot = slot
        require_cuda_f32(weight, bias, *srcs)
        L = lib()
        B, _, H, W = srcs[0].shape
        Cout, ks = weight.shape[0], weight.shape[2]
        Ho, Wo = _conv_out_size(H, ks, stride, pad), _conv_out_size(W, ks, stride, pad)
        if pack.stride != stride or pack.pad != pad:
            raise _lib.RsisHipError("PackedConv was built for stride %d pad %d, used with %d/%d" % (pack.stride, pack.pad, stride, pad))
        wp = pack.fwd(weight)
        out = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=weight.device)
        # 1x1 / stride s (the downsample convs of ResNet layers 2-4): run the stride-1 GEMM (LDS-DMA path) on a sub-sampled copy
        # of the input instead of the gather implicit GEMM, and keep THAT copy for the weight gradient (1/s^2 of the input,
        # tile-aligned for the LDS-DMA weight-gradient kernel).  Same packed weights: a 1x1 pack does not depend on the stride.
        ctx.in_shape = None
        if ks == 1 and stride > 1 and pad == 0 and nsrc == 1 and (SUBSAMPLE_1X1[0] or pack.dtype == DTYPE_BF16):
            ctx.in_shape = tuple(srcs[0].shape)
            sub = torch.empty((B, srcs[0].shape[1], Ho, Wo), dtype=torch.float32, device=weight.device)
            check(L.rsis_subsample2d(ptr(srcs[0]), ptr(sub), B * srcs[0].shape[1], H, W, stride, stream()), "rsis_subsample2d")
            srcs = [sub]
            H, W, stride_k = Ho, Wo, 1
        else:
            stride_k = stride
        # split-K (atomic, order-nondeterministic sums) only while training; inference stays bit-reproducible and keeps the
        # forward within the 1e-4 parity bar of the reference (the split sum moves the deepest skip conv by ~1e-5 relative)
        tile = FORCE_TILE[0] + (100 if pack.training_call else 0)
        check(L.rsis_conv2d_fwd(ptr_array(srcs), int_array([s.shape[1] for s in srcs]), nsrc, B, H, W, ptr(wp), Cout, ks, stride_k,
                                pad, ptr(bias.detach() if bias is not None else None), None, ptr(out), Ho, Wo, tile, pack.dtype, stream()),
              "rsis_conv2d_fwd")
        ctx.pack, ctx.stride, ctx.pad, ctx.nsrc = pack, stride, pad, nsrc
        ctx.has_bias = bias is not None
        ctx.wparam, ctx.bparam = weight, bias
        ctx.save_for_backward(weight, *srcs)
        return out

    @staticmethod
    def backward(ctx, dy):
        weight = ctx.saved_tensors[0]
        srcs = list(ctx.saved_tensors[1:])
        dy = _contig(dy)
        L = lib()
        ks = weight.shape[2]
        nsrc = ctx.nsrc
        grads = [None] * (nsrc + 2)
        take, park = ctx.slot if isinstance(ctx.slot, tuple) else (ctx.slot, None)
        addend = take.take() if take is not None else None
        sub = ctx.in_shape is not None            # srcs[0] is the sub-sampled copy of a strided 1x1 conv's input
        in_shapes = [ctx.in_shape] if sub else [tuple(t.shape) for t in srcs]
        if any(ctx.needs_input_grad[5:5 + nsrc]):
            wd = ctx.pack.dgrad(weight)
            inplace, extra = False, None
            if addend is not None:
                if nsrc != 1 or tuple(addend.shape) != in_shapes[0]:
                    raise _lib.RsisHipError("GradSlot: the parked gradient does not belong to this conv's input")
                if ctx.stride != 1:
                    if ks == 1 and ctx.pad == 0 and addend.is_contiguous():
                        inplace = True             # strided 1x1: accumulate into the parked tensor (no memset, no add)
                    else:
                        extra, addend = addend, None
            dxs = _dgrad_all(L, dy, wd, ctx.pack.cin, ks, ctx.stride, ctx.pad, in_shapes, in_shapes[0][2], in_shapes[0][3], addend,
                             inplace, dtype=ctx.pack.dtype)
            if extra is not None:
                dxs[0].add_(extra)
            for i in range(nsrc):
                if ctx.needs_input_grad[5 + i]:
                    grads[i] = dxs[i]
            if park is not None and nsrc == 1 and grads[0] is not None and park.park(grads[0]):
                grads[0] = None                    # conv1's data-gradient kernel adds it
        want_w = ctx.needs_input_grad[5 + nsrc]
        want_b = ctx.has_bias and ctx.needs_input_grad[6 + nsrc]
        if (want_w and want_b and weight.shape[0] == 1 and ks == 3 and ctx.stride == 1 and ctx.pad == 1 and nsrc == 1 and
                weight.shape[1] in (4, 8, 16) and srcs[0].shape[3] % 4 == 0):
            # conv_out: weight and bias gradient in one launch (rsis_conv_out_wgrad)
            tw, tb = _direct_target(ctx.wparam), _direct_target(ctx.bparam)
            dW = tw if tw is not None else torch.zeros_like(weight)
            db = tb if tb is not None else torch.zeros(1, dtype=torch.float32, device=dy.device)
            x0 = srcs[0]
            check(L.rsis_conv_out_wgrad(ptr(dy), ptr(x0), ptr(dW), ptr(db), x0.shape[0], x0.shape[1], x0.shape[2], x0.shape[3], stream()),
                  "rsis_conv_out_wgrad")
            grads[nsrc] = None if tw is not None else dW
            grads[nsrc + 1] = None if tb is not None else db
            return (None, None, None, None, None) + tuple(grads)
        if want_w:
            tgt = _direct_target(ctx.wparam)
            dW = _wgrad_all(L, dy, srcs, tuple(weight.shape), ks, 1 if sub else ctx.stride, ctx.pad, 0, out=tgt, dtype=ctx.pack.dtype)
            grads[nsrc] = None if tgt is not None else dW
        if want_b:
            tgt = _direct_target(ctx.bparam)
            db = tgt if tgt is not None else torch.zeros(weight.shape[0], dtype=torch.float32, device=dy.device)
            check(L.rsis_bias_grad(ptr(dy), ptr(db), dy.shape[0], dy.shape[1], dy.shape[2] * dy.shape[3], 0, stream()),
                  "rsis_bias_grad")
            grads[nsrc + 1] = None if tgt is not None else db
        return (None, None, None, None, None) + tuple(grads)


def conv2d(srcs, weight, bias, stride, pad, pack, grad_slot=None, park_slot=None):
    """nn.Conv2d over the channel concat of `srcs` (list of NCHW tensors).  grad_slot: the slot this conv's data gradient
    takes an addend from; park_slot: the slot it parks its own data gradient in (see GradSlot)."""
    # (ctx.needs_input_grad is True for parameters even under no_grad, and grad mode is off inside Function.forward, so the
    #  "is this a training call" decision is taken here)
    training = (torch.is_grad_enabled() and (weight.requires_grad or any(s.requires_grad for s in srcs))) or TRAINING_FORWARD[0]
    if pack.dtype == DTYPE_F32_WINO and not training and not WINOGRAD_INFER[0]:
        pack = pack.direct_twin()            # inference / parity path: the direct kernel, segmented accumulation (see WINOGRAD_INFER)
    pack.training_call = training
    if grad_slot is not None:
        grad_slot.reset()
    slot = grad_slot if park_slot is None else (grad_slot, park_slot)
    return _Conv2dFn.apply(pack, int(stride), int(pad), len(srcs), slot, *srcs, weight, bias)


# Inference: the eval-mode BatchNorm behind a conv (+ residual add) (+ ReLU) in the conv's epilogue (rsis_conv2d_fwd_bn_eval) -- bit for bit
# the two launches, without the BatchNorm's read + write of the activation.  RSIS_EVAL_FOLD=0 keeps the separate launches (A/B switch).
EVAL_FOLD = [os.environ.get("RSIS_EVAL_FOLD", "1") != "0"]
_ERR_UNSUPPORTED = 3


def conv2d_bn_eval(x, weight, bias, stride, pad, pack, gamma, beta, running_mean, running_var, eps, relu=False, res=None):
    """relu?(bn_eval(conv(x) + bias) + res) as ONE launch, for calls that record no autograd graph (test() / eval.py); returns None when the
    library has no folded epilogue for this conv (conv_out, output channels not a multiple of 4, a conv the bf16 kernels run, ...) -- the caller
    then runs conv and BatchNorm."""
    if not EVAL_FOLD[0] or torch.is_grad_enabled() or pack.dtype not in (DTYPE_F32, DTYPE_F32_WINO, DTYPE_BF16):
        return None                              # (a bf16 pack: only the convs the library runs on the fp32 kernels anyway -- it decides)
    if pack.dtype == DTYPE_F32_WINO:
        if WINOGRAD_INFER[0]:
            return None                          # opted into Winograd for inference: that kernel has no folded epilogue
        pack = pack.direct_twin()                # the inference path of a Winograd conv is the direct kernel (see conv2d)
    x = _contig(x)
    res = _contig(res) if res is not None else None
    require_cuda_f32(x, weight, bias, res, gamma, beta, running_mean, running_var)
    L = lib()
    B, Cin, H, W = x.shape
    Cout, ks = weight.shape[0], weight.shape[2]
    Ho, Wo = _conv_out_size(H, ks, stride, pad), _conv_out_size(W, ks, stride, pad)
    if pack.stride != stride or pack.pad != pad:
        raise _lib.RsisHipError("PackedConv was built for stride %d pad %d, used with %d/%d" % (pack.stride, pack.pad, stride, pad))
    if Cout % 4 != 0:
        return None
    pack.training_call = False
    wp = pack.fwd(weight)
    stride_k = stride
    if ks == 1 and stride > 1 and pad == 0:      # the strided 1x1 convs run the stride-1 GEMM on a sub-sampled copy (see _Conv2dFn)
        sub = torch.empty((B, Cin, Ho, Wo), dtype=torch.float32, device=x.device)
        check(L.rsis_subsample2d(ptr(x), ptr(sub), B * Cin, H, W, stride, stream()), "rsis_subsample2d")
        x, H, W, stride_k = sub, Ho, Wo, 1
    out = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    assert res is None or tuple(res.shape) == tuple(out.shape)
    rc = L.rsis_conv2d_fwd_bn_eval(ptr_array([x]), int_array([Cin]), 1, B, H, W, ptr(wp), Cout, ks, stride_k, pad,
                                   ptr(bias.detach() if bias is not None else None), ptr(res), ptr(gamma.detach()), ptr(beta.detach()),
                                   ptr(running_mean), ptr(running_var), float(eps), 1 if relu else 0, ptr(out), Ho, Wo, FORCE_TILE[0], pack.dtype, stream())
    if rc == _ERR_UNSUPPORTED:
        return None
    check(rc, "rsis_conv2d_fwd_bn_eval")
    return out


class _ConvLSTMFn(torch.autograd.Function):
    """ConvLSTMCell.forward (reference clstm.py:19-62) as one fused kernel; returns (h, c)."""

    @staticmethod
    def forward(ctx, pack, pad, nx, has_state, training, *tensors):
        xs = [_contig(t) for t in tensors[:nx]]
        h_prev, c_prev, weight, bias = tensors[nx], tensors[nx + 1], tensors[nx + 2], tensors[nx + 3]
        require_cuda_f32(weight, bias, h_prev, c_prev, *xs)
        L = lib()
        B, _, H, W = xs[0].shape
        hid, ks = weight.shape[0] // 4, weight.shape[2]
        srcs = list(xs)
        if has_state:
            h_prev, c_prev = _contig(h_prev), _contig(c_prev)
            srcs.append(h_prev)
        wp = pack.fwd(weight, bias)
        # (grad mode is off inside Function.forward and ctx.needs_input_grad is True for parameters even under no_grad: convlstm()
        #  decides whether this is a training call.  An inference call saves no gates -- act_out == NULL is what selects the
        #  segmented-accumulation kernel in the library)
        need_grad = training and any(ctx.needs_input_grad)
        h = torch.empty((B, hid, H, W), dtype=torch.float32, device=weight.device)
        c = torch.empty_like(h)
        act = torch.empty((B, 4 * hid, H, W), dtype=torch.float32, device=weight.device) if need_grad else None
        # zero state (clstm.py:26-37): the h_prev segment is the LAST segment of the packed K axis, so it is skipped
        # simply by passing the x sources only (the kernel walks the K-tiles of the sources it is given).
        segs = [s.shape[1] for s in srcs]
        check(L.rsis_convlstm_fwd(ptr_array(srcs), int_array(segs), len(srcs), B, H, W, ptr(wp), ptr(pack.bias_p), None,
                                  ptr(c_prev) if has_state else None, ptr(h), ptr(c), ptr(act), hid, ks, pad, FORCE_TILE[0], pack.dtype,
                                  stream()), "rsis_convlstm_fwd")
        ctx.pack, ctx.pad, ctx.nx, ctx.has_state = pack, pad, nx, has_state
        if need_grad:
            ctx.save_for_backward(weight, act, c, c_prev if has_state else None, *srcs)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        weight, act, c, c_prev = ctx.saved_tensors[:4]
        srcs = list(ctx.saved_tensors[4:])
        L = lib()
        nx, has_state = ctx.nx, ctx.has_state
        B, hid, H, W = c.shape
        ks = weight.shape[2]
        dh = _contig(dh) if dh is not None else None
        dc = _contig(dc) if dc is not None else None
        da = torch.empty_like(act)
        dc_prev = torch.empty_like(c) if has_state else None
        check(L.rsis_convlstm_bwd_gates(ptr(dh), None, ptr(dc), ptr(act), ptr(c_prev), ptr(c), ptr(da), ptr(dc_prev), None, B, hid, H * W,
                                        stream()), "rsis_convlstm_bwd_gates")
        grads = [None] * (nx + 4)
        need_src = list(ctx.needs_input_grad[5:5 + nx]) + ([ctx.needs_input_grad[5 + nx]] if has_state else [])
        if any(need_src):
            wd = ctx.pack.dgrad(weight)
            dxs = _dgrad_all(L, da, wd, ctx.pack.cin, ks, 1, ctx.pad, srcs, H, W, dtype=ctx.pack.dtype)
            for i in range(nx):
                if need_src[i]:
                    grads[i] = dxs[i]
            if has_state and need_src[nx]:
                grads[nx] = dxs[nx]
        if has_state:
            grads[nx + 1] = dc_prev
        if ctx.needs_input_grad[5 + nx + 2]:
            # zero state: the h_prev channels of dW get no contribution (h_prev == 0)
            grads[nx + 2] = _wgrad_all(L, da, srcs, tuple(weight.shape), ks, 1, ctx.pad, hid, dtype=ctx.pack.dtype)
        if ctx.needs_input_grad[5 + nx + 3]:
            db = torch.zeros(4 * hid, dtype=torch.float32, device=da.device)
            check(L.rsis_bias_grad(ptr(da), ptr(db), B, 4 * hid, H * W, hid, stream()), "rsis_bias_grad")
            grads[nx + 3] = db
        return (None, None, None, None, None) + tuple(grads)


def convlstm(xs, state, weight, bias, pad, pack):
    """xs: list of NCHW tensors whose channel concat is the cell input; state: None or (h, c)."""
    has_state = state is not None
    h_prev, c_prev = (state[0], state[1]) if has_state else (None, None)
    training = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in list(xs) + [h_prev, c_prev, weight, bias])
    return _ConvLSTMFn.apply(pack, int(pad), len(xs), has_state, training, *xs, h_prev, c_prev, weight, bias)


class _UpsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo):
        x = _contig(x)
        require_cuda_f32(x)
        B, C, Hi, Wi = x.shape
        y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
        check(lib().rsis_upsample_bilinear_ac_fwd(ptr(x), ptr(y), B * C, Hi, Wi, Ho, Wo, stream()), "rsis_upsample_fwd")
        ctx.dims = (B, C, Hi, Wi, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, Hi, Wi, Ho, Wo = ctx.dims
        dy = _contig(dy)
        dx = torch.empty((B, C, Hi, Wi), dtype=torch.float32, device=dy.device)
        check(lib().rsis_upsample_bilinear_ac_bwd(ptr(dy), ptr(dx), B * C, Hi, Wi, Ho, Wo, stream()), "rsis_upsample_bwd")
        return dx, None, None


def upsample_bilinear_ac(x, size):
    """nn.UpsamplingBilinear2d(size=size) (align_corners=True)."""
    Ho, Wo = int(size[0]), int(size[1])
    if x.shape[2] == Ho and x.shape[3] == Wo:
        return x  # align_corners resize to the same size is the identity
    return _UpsampleFn.apply(x, Ho, Wo)


class _GlobalMaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _contig(x)
        require_cuda_f32(x)
        B, C, H, W = x.shape
        y = torch.empty((B, C, 1, 1), dtype=torch.float32, device=x.device)
        arg = torch.empty((B, C), dtype=torch.int32, device=x.device)
        check(lib().rsis_global_maxpool_fwd(ptr(x), ptr(y), ptr(arg), B * C, H * W, stream()), "rsis_global_maxpool_fwd")
        ctx.save_for_backward(arg)
        ctx.dims = (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        B, C, H, W = ctx.dims
        dy = _contig(dy)
        dx = torch.empty((B, C, H, W), dtype=torch.float32, device=dy.device)
        check(lib().rsis_global_maxpool_bwd(ptr(dy), ptr(arg), ptr(dx), B * C, H * W, stream()), "rsis_global_maxpool_bwd")
        return dx


def global_maxpool(x):
    """nn.MaxPool2d(kernel = full map) -> (B, C, 1, 1)."""
    return _GlobalMaxPoolFn.apply(x)


class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, running_mean, running_var, train, relu, eps, momentum, arena, res_slot=None, want_grad=True):
        x = _contig(x)
        ctx.res_slot = res_slot
        res = _contig(res) if res is not None else None
        require_cuda_f32(x, res, gamma, beta, running_mean, running_var)
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        flags = int(train)
        if train:
            if arena is not None:      # (fwd stats, bwd stats) slices of an arena the caller zeroed for this iteration
                stats, flags = arena[0], flags | 2
            else:
                stats = torch.empty(2 * C, dtype=torch.float64, device=x.device)
            mean = torch.empty(C, dtype=torch.float32, device=x.device)
            rstd = torch.empty_like(mean)
        else:
            stats = mean = rstd = None
        # with ReLU on float4-able planes the forward leaves the ReLU mask as bytes (one per 4 elements) and the backward reads
        # those instead of y: 1/16 of the bytes for the same bits (rsis_bn_*_mask); otherwise y is kept.  No mask is written when
        # nothing will be back-propagated (want_grad, decided in batchnorm(): grad mode is off in here and ctx.needs_input_grad is
        # True for parameters even under no_grad).
        ctx.masked = bool(relu) and (H * W) % 4 == 0 and want_grad
        if ctx.masked:
            keep = torch.empty(x.numel() // 4, dtype=torch.uint8, device=x.device)
            check(lib().rsis_bn_fwd_mask(ptr(x), ptr(res), ptr(y), ptr(keep), ptr(stats), ptr(gamma.detach()), ptr(beta.detach()),
                                         ptr(running_mean), ptr(running_var), ptr(mean), ptr(rstd), B, C, H * W, float(eps),
                                         float(momentum), flags, stream()), "rsis_bn_fwd_mask")
        else:
            keep = y if relu else None
            check(lib().rsis_bn_fwd(ptr(x), ptr(res), ptr(y), ptr(stats), ptr(gamma.detach()), ptr(beta.detach()), ptr(running_mean),
                                    ptr(running_var), ptr(mean), ptr(rstd), B, C, H * W, float(eps), float(momentum), int(relu),
                                    flags, stream()), "rsis_bn_fwd")
        ctx.train, ctx.relu, ctx.has_res, ctx.eps = train, relu, res is not None, eps
        ctx.arena, ctx.gparam, ctx.bparam = arena, gamma, beta
        if train:
            ctx.save_for_backward(x, keep, gamma, mean, rstd)
        else:
            ctx.save_for_backward(x, keep, gamma, running_mean, running_var)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, mean, rstd = ctx.saved_tensors      # y: the forward output, or its ReLU mask bytes (ctx.masked)
        dy = _contig(dy)
        B, C, H, W = x.shape
        if not ctx.train:
            # eval-mode BN is an affine map with constant statistics: dx = g * gamma / sqrt(running_var + eps) (rsis_bn_bwd_eval;
            # here `mean` / `rstd` hold running_mean / running_var)
            stats = torch.empty(2 * C, dtype=torch.float64, device=dy.device)
            dx = torch.empty_like(x)
            need_dres = ctx.has_res and ctx.relu
            dres = torch.empty_like(x) if need_dres else None
            dgamma = torch.empty(C, dtype=torch.float32, device=dy.device)
            dbeta = torch.empty_like(dgamma)
            fn, name = (lib().rsis_bn_bwd_eval_mask, "rsis_bn_bwd_eval_mask") if ctx.masked else (lib().rsis_bn_bwd_eval, "rsis_bn_bwd_eval")
            check(fn(ptr(dy), ptr(x), ptr(y), ptr(mean), ptr(rstd), ptr(gamma.detach()), ptr(stats), ptr(dx), ptr(dres),
                     ptr(dgamma), ptr(dbeta), B, C, H * W, float(ctx.eps), int(ctx.relu), stream()), name)
            if ctx.has_res and not need_dres:
                dres = dy
            return dx, dres, dgamma, dbeta, None, None, None, None, None, None, None, None, None
        flags = int(ctx.relu)
        if ctx.arena is not None:
            stats, flags = ctx.arena[1], flags | 2
        else:
            stats = torch.empty(2 * C, dtype=torch.float64, device=dy.device)
        dx = torch.empty_like(x)
        need_dres = ctx.has_res and ctx.relu
        dres = torch.empty_like(x) if need_dres else None
        tg, tb = _direct_target(ctx.gparam), _direct_target(ctx.bparam)
        direct = tg is not None and tb is not None
        if direct:
            dgamma, dbeta, flags = tg, tb, flags | 4
        else:
            dgamma = torch.empty(C, dtype=torch.float32, device=dy.device)
            dbeta = torch.empty_like(dgamma)
        fn, name = (lib().rsis_bn_bwd_mask, "rsis_bn_bwd_mask") if ctx.masked else (lib().rsis_bn_bwd, "rsis_bn_bwd")
        check(fn(ptr(dy), ptr(x), ptr(y), ptr(mean), ptr(rstd), ptr(gamma.detach()), ptr(stats), ptr(dx), ptr(dres),
                 ptr(dgamma), ptr(dbeta), B, C, H * W, flags, stream()), name)
        if ctx.has_res and not need_dres:
            dres = dy
        if direct:
            dgamma = dbeta = None
        if ctx.res_slot is not None and ctx.res_slot.park(dres):
            dres = None                                # picked up by the data-gradient kernel of the block's first conv
        return dx, dres, dgamma, dbeta, None, None, None, None, None, None, None, None, None


def batchnorm(x, gamma, beta, running_mean, running_var, train, relu=False, res=None, eps=1e-5, momentum=0.1, arena=None,
              res_slot=None):
    """nn.BatchNorm2d (+ residual add) (+ ReLU): y = act(bn(x) + res).  arena: optional (fwd, bwd) float64 [2*C] scratch
    slices that the caller zeroed for this iteration (saves one memset per layer per pass)."""
    want_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, res, gamma, beta))
    return _BatchNormFn.apply(x, res, gamma, beta, running_mean, running_var, bool(train), bool(relu), eps, momentum, arena,
                              res_slot if (train and res is not None) else None, want_grad)


class _MaxPool3x3s2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slot=None):
        ctx.slot = slot
        x = _contig(x)
        require_cuda_f32(x)
        B, C, H, W = x.shape
        Ho, Wo = _conv_out_size(H, 3, 2, 1), _conv_out_size(W, 3, 2, 1)
        y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
        arg = torch.empty((B, C, Ho, Wo), dtype=torch.uint8, device=x.device)
        check(lib().rsis_maxpool3x3s2_fwd(ptr(x), ptr(y), ptr(arg), B * C, H, W, Ho, Wo, stream()), "rsis_maxpool3x3s2_fwd")
        ctx.save_for_backward(arg)
        ctx.dims = (B, C, H, W, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        B, C, H, W, Ho, Wo = ctx.dims
        dy = _contig(dy)
        parked = ctx.slot.take() if ctx.slot is not None else None
        if parked is not None and (tuple(parked.shape) != (B, C, H, W) or not parked.is_contiguous()):
            raise _lib.RsisHipError("GradSlot: the parked gradient does not belong to this max-pool's input")
        dx = parked if parked is not None else torch.empty((B, C, H, W), dtype=torch.float32, device=dy.device)
        check(lib().rsis_maxpool3x3s2_bwd(ptr(dy), ptr(arg), ptr(dx), B * C, H, W, Ho, Wo, 1 if parked is not None else 0, stream()),
              "rsis_maxpool3x3s2_bwd")
        return dx, None


def maxpool3x3s2(x, grad_slot=None):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1).  grad_slot: a GradSlot holding the gradient x receives from another
    consumer (parked by ops.grad_tap); the backward accumulates into it in place instead of autograd adding the two."""
    if grad_slot is not None:
        grad_slot.reset()
    return _MaxPool3x3s2Fn.apply(x, grad_slot)


def adam_step_flat(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, gscale=1.0, step_dev=None, bump=True):
    """torch.optim.Adam step on flat fp32 buffers (in place; bumps the packed-weight epoch).  step_dev: optional int32 device
    tensor (one element) holding the update count -- read by the kernel instead of `step` (hipGraph replay)."""
    require_cuda_f32(p, g, m, v)
    check(lib().rsis_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                               float(weight_decay), int(step), float(gscale), ptr(step_dev), stream()), "rsis_adam_step")
    if bump:
        bump_weight_epoch()


def _require_flat(what, *ts):
    """equal-length contiguous ranges: the kernel walks all of them with the first one's length"""
    require_cuda_f32(*ts)
    if any(t.numel() != ts[0].numel() or not t.is_contiguous() for t in ts):
        raise ValueError("%s: the parameter, gradient and state ranges must be contiguous and of one length" % what)


def sgd_step_flat(p, g, buf, lr, momentum, weight_decay, gscale=1.0, bump=True):
    """torch.optim.SGD(momentum) step on flat fp32 buffers (in place; bumps the packed-weight epoch).  buf: the momentum buffer,
    zero before the first step of its parameters."""
    _require_flat("sgd_step_flat", p, g, buf)
    check(lib().rsis_sgd_step(ptr(p), ptr(g), ptr(buf), p.numel(), float(lr), float(momentum), float(weight_decay), float(gscale),
                              stream()), "rsis_sgd_step")
    if bump:
        bump_weight_epoch()


def rmsprop_step_flat(p, g, sq, lr, alpha, eps, weight_decay, gscale=1.0, bump=True):
    """torch.optim.RMSprop step on flat fp32 buffers (in place; bumps the packed-weight epoch).  sq: the square average."""
    _require_flat("rmsprop_step_flat", p, g, sq)
    check(lib().rsis_rmsprop_step(ptr(p), ptr(g), ptr(sq), p.numel(), float(lr), float(alpha), float(eps), float(weight_decay),
                                  float(gscale), stream()), "rsis_rmsprop_step")
    if bump:
        bump_weight_epoch()


def assign_min_cost(scores):
    """Device-side Hungarian matching (reference hungarian.py:91-125): scores (B, G, T) fp32, rows = GT slots, columns =
    predictions -> perm (B, G) int64, perm[b, t] = GT slot matched to prediction t (0 in the unassigned tail)."""
    scores = _contig(scores)
    require_cuda_f32(scores)
    B, G, T = scores.shape
    perm = torch.empty((B, G), dtype=torch.int64, device=scores.device)
    check(lib().rsis_assign_min_cost(ptr(scores), ptr(perm), B, G, T, stream()), "rsis_assign_min_cost")
    return perm


def softiou_supported(out_masks, y_mask):
    """the fused soft-IoU kernels cover 1 <= T <= 128 predictions, 1 <= G <= 128 ground-truth slots and N % 8 == 0 pixels"""
    return (out_masks.is_cuda and out_masks.dtype == torch.float32 and y_mask.dtype == torch.float32 and
            1 <= out_masks.size(1) <= 128 and 1 <= y_mask.size(1) <= 128 and out_masks.size(2) >= 8 and out_masks.size(2) % 8 == 0)


def _ignore_map(ignore, B, N, device):
    """the (B, N) uint8 ignore map as the soft-IoU kernels read it: contiguous, on the device, 4-byte aligned (a lane's four pixels are
    one word); None stays None"""
    if ignore is None:
        return None
    if ignore.dtype != torch.uint8 or ignore.device != device or tuple(ignore.shape) != (B, N):
        raise ValueError("ignore map: uint8 (%d, %d) on %s expected, got %s %s on %s" % (B, N, device, ignore.dtype, tuple(ignore.shape), ignore.device))
    ignore = _contig(ignore)
    return ignore.clone() if ignore.data_ptr() % 4 else ignore


def softiou_sums(out_masks, y_mask, ignore=None):
    """S (B, T+1, G+1): intersections sigmoid(out_masks[b,t]) . y_mask[b,g], plus the row / column of plain sums
    (include/rsis_hip.h: rsis_softiou_sums).  ignore: (B, N) uint8, non-zero = the pixel is left out of every sum
    (rsis_softiou_sums_ignore); None = the plain entry point.  No gradient."""
    out_masks, y_mask = _contig(out_masks.detach()), _contig(y_mask)
    require_cuda_f32(out_masks, y_mask)
    B, T, N = out_masks.shape
    G = y_mask.shape[1]
    S = torch.empty((B, T + 1, G + 1), dtype=torch.float32, device=out_masks.device)
    if ignore is None:
        check(lib().rsis_softiou_sums(ptr(out_masks), ptr(y_mask), ptr(S), B, T, G, N, stream()), "rsis_softiou_sums")
    else:
        ignore = _ignore_map(ignore, B, N, out_masks.device)
        check(lib().rsis_softiou_sums_ignore(ptr(out_masks), ptr(y_mask), ptr(ignore), ptr(S), B, T, G, N, stream()), "rsis_softiou_sums_ignore")
    return S


def softiou_cost_matrix(S, e=1e-6):
    """all-pairs cost (B, G, T) of reference train.py:102-110 from the sums: 1 - I / (sum p + sum y - I + e)"""
    inter = S[:, :-1, :-1]                                   # (B, T, G)
    den = S[:, :-1, -1:] + S[:, -1:, :-1] - inter + e
    return (1 - inter / den).transpose(1, 2)


class _SoftIoUMatchedFn(torch.autograd.Function):
    """cost[b, t] = softIoU(y_mask[b, perm[b, t]], out_masks[b, t]) (hungarian.py:62-89) from the precomputed sums S;
    the backward is one elementwise kernel over the logits."""

    @staticmethod
    def forward(ctx, out_masks, y_mask, perm, S, e, ignore=None):
        B, T, N = out_masks.shape
        idx = perm[:, :T]
        inter = torch.gather(S[:, :T, :-1], 2, idx.unsqueeze(-1)).squeeze(-1)          # (B, T)
        ysum = torch.gather(S[:, -1, :-1], 1, idx)
        den = S[:, :T, -1] + ysum - inter + e
        ctx.has_ignore = ignore is not None
        ctx.save_for_backward(*((out_masks, y_mask, perm, inter, den) + ((ignore,) if ignore is not None else ())))
        return 1 - inter / den

    @staticmethod
    def backward(ctx, g):
        out_masks, y_mask, perm, inter, den = ctx.saved_tensors[:5]
        B, T, N = out_masks.shape
        g = g.contiguous().float()
        ca = (-g / den).contiguous()
        cb = (g * inter / (den * den)).contiguous()
        logits = _contig(out_masks.detach())
        d = torch.empty_like(logits)
        if ctx.has_ignore:
            check(lib().rsis_softiou_bwd_ignore(ptr(logits), ptr(y_mask), ptr(ctx.saved_tensors[5]), ptr(perm), perm.shape[1], ptr(ca), ptr(cb),
                                                ptr(d), B, T, y_mask.shape[1], N, stream()), "rsis_softiou_bwd_ignore")
        else:
            check(lib().rsis_softiou_bwd(ptr(logits), ptr(y_mask), ptr(perm), perm.shape[1], ptr(ca), ptr(cb), ptr(d), B, T,
                                         y_mask.shape[1], N, stream()), "rsis_softiou_bwd")
        return d, None, None, None, None, None


def softiou_matched(out_masks, y_mask, perm, S, e=1e-6, ignore=None):
    """(B, T) soft-IoU cost of every prediction against its matched ground-truth mask; differentiable w.r.t. out_masks.
    ignore: the map S was computed with (softiou_sums): the gradient is zero at its pixels."""
    y_mask, perm = _contig(y_mask), _contig(perm)
    if ignore is None:
        return _SoftIoUMatchedFn.apply(out_masks, y_mask, perm, S, float(e))
    ignore = _ignore_map(ignore, out_masks.shape[0], out_masks.shape[2], out_masks.device)
    return _SoftIoUMatchedFn.apply(out_masks, y_mask, perm, S, float(e), ignore)


# ---- THE rule that picks the heads kernels (csrc/losses.hip), asked by _HeadsFn and by decoder_seq's forward heads and
# _heads_bwd_all_steps: the kernels of rsis_heads_fwd / rsis_heads_bwd whenever they accept the call -- what ran before the wide family
# existed keeps its bits -- and the wide family (rsis_heads_wide_*) otherwise.  The limits restate rsis_l_heads_* (losses.hip).
HEADS_MAXK, HEADS_MAXC, HEADS_WIDE_MAXC, HEADS_LDS_FLOATS = 2048, 64, 1024, 64 * 1024 // 4


def heads_family(rows, K, ncls, backward=False):
    """"small", "wide" or None (no kernel takes the call) for `rows` rows of K features and ncls classes; backward: rsis_heads_bwd also
    needs 2 rows (ncls + 1) + rows ceil(K / rows) floats of LDS within 64 KB"""
    if not (rows >= 1 and 1 <= K <= HEADS_MAXK and 1 <= ncls <= HEADS_WIDE_MAXC):
        return None
    if ncls <= HEADS_MAXC and (not backward or 2 * rows * (ncls + 1) + rows * ((K + rows - 1) // rows) <= HEADS_LDS_FLOATS):
        return "small"
    return "wide"


def heads_fwd_launch(L, sides, Cs, rows, Wc, bc, Ws, bs, probs, stop, keys=None):
    """the forward heads of `rows` rows on the family heads_family picks.  sides: the per-level feature tensors (with keys: where the
    launch writes them); keys = (per-level key tensors, per-level arg-max tensors)"""
    ncls, n = Wc.shape[0], len(Cs)
    fam = heads_family(rows, sum(Cs), ncls)
    w = (ptr(Wc.detach()), ptr(bc.detach()), ncls, ptr(Ws.detach()), ptr(bs.detach()), ptr(probs), ptr(stop), stream())
    if fam == "wide":
        if keys is not None:
            check(L.rsis_heads_wide_fwd(ptr_array(keys[0]), ptr_array(sides), ptr_array(keys[1]), None, int_array(Cs), n, rows, *w), "rsis_heads_wide_fwd(keys)")
        else:
            check(L.rsis_heads_wide_fwd(None, None, None, ptr_array(sides), int_array(Cs), n, rows, *w), "rsis_heads_wide_fwd")
    elif keys is not None:      # (fam None: the small entry point reports the refusal)
        check(L.rsis_heads_fwd_keys(ptr_array(keys[0]), ptr_array(sides), ptr_array(keys[1]), int_array(Cs), n, rows, *w), "rsis_heads_fwd_keys")
    else:
        check(L.rsis_heads_fwd(ptr_array(sides), int_array(Cs), n, rows, *w), "rsis_heads_fwd")


def heads_bwd_launch(L, sides, Cs, rows, Wc, Ws, probs, dprobs, dstop, dsides, hb, wide):
    """one backward call over `rows` rows: rsis_heads_bwd, or (wide) the launch pair of rsis_heads_wide_bwd with its scratch"""
    ncls = Wc.shape[0]
    a = (ptr_array(sides), int_array(Cs), len(Cs), rows, ptr(Wc.detach()), ncls, ptr(Ws.detach()), ptr(probs), ptr(dprobs), ptr(dstop),
         ptr_array(dsides), ptr(hb[0]), ptr(hb[1]), ptr(hb[2]), ptr(hb[3]))
    if not wide:
        return L.rsis_heads_bwd(*a, stream())
    scratch = torch.empty(rows * (ncls + 1), dtype=torch.float32, device=Wc.device)
    return L.rsis_heads_wide_bwd(*a, ptr(scratch), scratch.numel(), stream())


class _HeadsFn(torch.autograd.Function):
    """class_probs, stop = softmax(fc_class(cat(sides))), fc_stop(cat(sides))  (reference model.py:169-182) in one launch each
    way; the concatenation is by pointer and the parameter gradients accumulate in place when DIRECT_GRAD is on."""

    @staticmethod
    def forward(ctx, n, *tensors):
        keys = tensors[n + 4] if len(tensors) > n + 4 else None
        if keys is not None:          # the features arrive as max-pool keys; this launch writes them (and the arg-max) into place
            assert all(t.is_contiguous() for t in tensors[:n])
            sides = [t.view(t.shape[0], -1) for t in tensors[:n]]
        else:
            sides = [_contig(t).reshape(t.shape[0], -1) for t in tensors[:n]]
        Wc, bc, Ws, bs = tensors[n:n + 4]
        require_cuda_f32(Wc, bc, Ws, bs, *sides)
        B, ncls = sides[0].shape[0], Wc.shape[0]
        probs = torch.empty((B, ncls), dtype=torch.float32, device=Wc.device)
        stop = torch.empty((B, 1), dtype=torch.float32, device=Wc.device)
        heads_fwd_launch(lib(), sides, [s.shape[1] for s in sides], B, Wc, bc, Ws, bs, probs, stop, keys)
        ctx.n = n
        ctx.extra = len(tensors) - (n + 4)
        ctx.shapes = [tuple(t.shape) for t in tensors[:n]]
        ctx.params = (Wc, bc, Ws, bs)
        ctx.save_for_backward(probs, Wc, Ws, *sides)
        return probs, stop

    @staticmethod
    def backward(ctx, dprobs, dstop):
        probs, Wc, Ws = ctx.saved_tensors[:3]
        sides = list(ctx.saved_tensors[3:])
        n = ctx.n
        B, ncls = probs.shape
        dprobs = _contig(dprobs) if dprobs is not None else None
        dstop = _contig(dstop) if dstop is not None else None
        dsides = [torch.empty_like(s) if ctx.needs_input_grad[1 + i] else None for i, s in enumerate(sides)]
        outs, tgts = [], []
        for j, p in enumerate(ctx.params):
            if ctx.needs_input_grad[1 + n + j]:
                t = _direct_target(p)
                tgts.append(t)
                outs.append(t if t is not None else torch.zeros_like(p))
            else:
                tgts.append(None)
                outs.append(None)
        Cs = [s.shape[1] for s in sides]
        wide = heads_family(B, sum(Cs), ncls, backward=True) == "wide"
        check(heads_bwd_launch(lib(), sides, Cs, B, Wc, Ws, probs, dprobs, dstop, dsides, outs, wide), "rsis_heads_wide_bwd" if wide else "rsis_heads_bwd")
        grads = [d.reshape(sh) if d is not None else None for d, sh in zip(dsides, ctx.shapes)]
        grads += [None if t is not None else o for t, o in zip(tgts, outs)]
        return (None,) + tuple(grads) + (None,) * ctx.extra


def heads_supported(sides, fc_class, fc_stop, min_rows=2):
    """the heads run on the kernels (heads_family: either family).  A single row is left to the callers that ask for it (min_rows=1,
    the sequence decoder): single-step RSIS.forward keeps the reference's 1-D outputs at B == 1 (model.py:169-182)"""
    return (sides[0].is_cuda and sides[0].shape[0] >= min_rows and len(sides) <= 5 and fc_stop.weight.shape[0] == 1 and
            fc_class.bias is not None and fc_stop.bias is not None and
            heads_family(sides[0].shape[0], fc_class.weight.shape[1], fc_class.weight.shape[0]) is not None)


def heads(sides, fc_class, fc_stop, keys=None):
    """(class_probs (B, ncls), stop logits (B, 1)) of reference RSIS.forward's tail from the list of pooled side features.
    keys = (per-level [B][C] int64 max-pool keys, per-level [B][C] int32 arg-max buffers): the features are still packed keys
    (rsis_lstm_job.side_key); the launch decodes them into `sides` / the arg-max buffers before it uses them."""
    if keys is not None:
        return _HeadsFn.apply(len(sides), *sides, fc_class.weight, fc_class.bias, fc_stop.weight, fc_stop.bias, keys)
    return _HeadsFn.apply(len(sides), *sides, fc_class.weight, fc_class.bias, fc_stop.weight, fc_stop.bias)


class _LossTailFn(torch.autograd.Function):
    """(total, [iou, stop, class]) of reference train.py:159-176 from class probabilities (B, T, C), matched class targets
    (B, T), stop logits (B, T), matched soft-IoU costs (B, T) and the two sample-weight matrices; one launch each way."""

    @staticmethod
    def forward(ctx, probs, y_class, stop, siou, sw_mask, sw_class, cls_w, bw, w_iou, w_cls, w_stop):
        probs, stop, siou = _contig(probs), _contig(stop), _contig(siou)
        y_class, sw_mask, sw_class = _contig(y_class), _contig(sw_mask), _contig(sw_class)
        require_cuda_f32(probs, stop, siou, sw_mask, sw_class, cls_w)
        n, C = y_class.numel(), probs.shape[-1]
        out = torch.empty(4, dtype=torch.float32, device=probs.device)
        check(lib().rsis_loss_tail(ptr(probs), ptr(y_class), ptr(stop), ptr(siou), ptr(sw_mask), ptr(sw_class), ptr(cls_w), n, C,
                                   float(bw), float(w_iou), float(w_cls), float(w_stop), ptr(out), None, None, None, None, stream()),
              "rsis_loss_tail")
        ctx.save_for_backward(probs, y_class, stop, siou, sw_mask, sw_class, cls_w)
        ctx.cfg = (n, C, float(bw), float(w_iou), float(w_cls), float(w_stop))
        total, parts = out[0], out[1:]
        ctx.mark_non_differentiable(parts)
        return total, parts

    @staticmethod
    def backward(ctx, g, _gparts):
        probs, y_class, stop, siou, sw_mask, sw_class, cls_w = ctx.saved_tensors
        n, C, bw, w_iou, w_cls, w_stop = ctx.cfg
        g = _contig(g.reshape(1).float())
        dprobs, dstop, dsiou = torch.empty_like(probs), torch.empty_like(stop), torch.empty_like(siou)
        check(lib().rsis_loss_tail(ptr(probs), ptr(y_class), ptr(stop), ptr(siou), ptr(sw_mask), ptr(sw_class), ptr(cls_w), n, C, bw, w_iou,
                                   w_cls, w_stop, None, ptr(dprobs), ptr(dstop), ptr(dsiou), ptr(g), stream()), "rsis_loss_tail(bwd)")
        return dprobs, None, dstop, dsiou, None, None, None, None, None, None, None


def loss_tail(probs, y_class, stop, siou, sw_mask, sw_class, cls_w, bw, w_iou, w_cls, w_stop):
    """bw: BCE balance weight or None (taken from the targets); cls_w: per-class weights tensor or None"""
    return _LossTailFn.apply(probs, y_class, stop, siou, sw_mask, sw_class, cls_w, -1.0 if bw is None else bw, w_iou, w_cls, w_stop)


# ---------------------------------------------------------------------------------------------------------------------------
# channel-blocked bf16 activations ("blk": logical [B][C][H][W] stored as bf16 [B][C/8][H][W][8]; csrc/conv_blk.hip) -- raw ops
# (no autograd): the blocked trunk's autograd functions are built on them
# ---------------------------------------------------------------------------------------------------------------------------
def blk_from_nchw(x):
    require_cuda_f32(x)
    x = _contig(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C // 8, H, W, 8), dtype=torch.bfloat16, device=x.device)
    check(lib().rsis_blk_from_nchw(ptr(x), ptr(y), B, C, H, W, stream()), "rsis_blk_from_nchw")
    return y


def blk_to_nchw(x):
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 5 and x.shape[-1] == 8
    B, Cb, H, W, _ = x.shape
    y = torch.empty((B, Cb * 8, H, W), dtype=torch.float32, device=x.device)
    check(lib().rsis_blk_to_nchw(ptr(x), ptr(y), B, Cb * 8, H, W, stream()), "rsis_blk_to_nchw")
    return y


def blk_conv2d(x, wp, cout, ks, variant=0, addend=None, bn=None, relu=False, single_rounding=False):
    """conv (stride 1, same padding, no bias) of a blk tensor with a bf16 pack (PackedConv(dtype=DTYPE_BF16).fwd / .dgrad);
    addend: a blk tensor of the output's shape, added before the rounding; bn = (gamma, beta, running_mean, running_var, eps) (+ relu): the
    eval-mode BatchNorm of the output in the conv's epilogue (rsis_blk_conv2d_bn_eval: inference)"""
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 5 and x.shape[-1] == 8 and cout % 8 == 0
    B, Cb, H, W, _ = x.shape
    y = torch.empty((B, cout // 8, H, W, 8), dtype=torch.bfloat16, device=x.device)
    assert addend is None or (addend.dtype == torch.bfloat16 and addend.is_contiguous() and tuple(addend.shape) == tuple(y.shape))
    if bn is None:
        check(lib().rsis_blk_conv2d(ptr(x), B, Cb * 8, H, W, ptr(wp), cout, ks, ptr(addend), ptr(y), int(variant), stream()), "rsis_blk_conv2d")
    else:
        g, b, m, v, eps = bn
        for t in (g, b, m, v):
            assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == cout
        check(lib().rsis_blk_conv2d_bn_eval(ptr(x), B, Cb * 8, H, W, ptr(wp), cout, ks, ptr(addend), ptr(g), ptr(b), ptr(m), ptr(v), float(eps),
                                            1 if relu else 0, 1 if single_rounding else 0, ptr(y), int(variant), stream()), "rsis_blk_conv2d_bn_eval")
    return y


def _blk_ok(*ts):
    for t in ts:
        assert t is None or (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and t.dim() == 5 and t.shape[-1] == 8), "blk tensor expected"


_BLK_SCRATCH = {}


def _blk_scratch(C, device):
    """per-split partial sums of the blk BatchNorm kernels: one buffer per (device, stream) -- launches on a stream are ordered"""
    key = (device, torch.cuda.current_stream().cuda_stream)
    n = lib().rsis_blk_bn_scratch_doubles(int(C))
    buf = _BLK_SCRATCH.get(key)
    if buf is None or buf.numel() < n:
        buf = _BLK_SCRATCH[key] = torch.empty(max(n, 64 * 2048 * 2), dtype=torch.float64, device=device)
    return buf


def blk_bn_fwd(x, res, gamma, beta, run_mean, run_var, eps, momentum, relu, train):
    """(y, save_mean, save_rstd) -- BatchNorm2d (+ res) (+ ReLU) on a blk tensor (rsis_blk_bn_fwd)"""
    _blk_ok(x, res)
    B, Cb, H, W, _ = x.shape
    C = Cb * 8
    y = torch.empty_like(x)
    sm = torch.empty(C, dtype=torch.float32, device=x.device) if train else None
    sr = torch.empty(C, dtype=torch.float32, device=x.device) if train else None
    check(lib().rsis_blk_bn_fwd(ptr(x), ptr(res), ptr(y), ptr(_blk_scratch(C, x.device)) if train else None, ptr(gamma), ptr(beta), ptr(run_mean),
                                ptr(run_var), ptr(sm), ptr(sr), B, C, H, W, float(eps), float(momentum), int(bool(relu)), int(bool(train)),
                                stream()), "rsis_blk_bn_fwd")
    return y, sm, sr


def blk_bn_bwd(dy, x, y, gamma, beta, save_mean, save_rstd, relu, want_dres, dgamma=None, dbeta=None, accumulate=False):
    """(dx, dres or None, dgamma, dbeta) of the train-mode blk BatchNorm (rsis_blk_bn_bwd)"""
    _blk_ok(dy, x, y)
    B, Cb, H, W, _ = x.shape
    C = Cb * 8
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        accumulate = False
    check(lib().rsis_blk_bn_bwd(ptr(dy), ptr(x), ptr(y), ptr(_blk_scratch(C, x.device)), ptr(gamma), ptr(beta), ptr(save_mean), ptr(save_rstd),
                                ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), int(bool(accumulate)), B, C, H, W, int(bool(relu)), stream()),
          "rsis_blk_bn_bwd")
    return dx, dres, dgamma, dbeta


def blk_subsample(x, stride):
    _blk_ok(x)
    B, Cb, H, W, _ = x.shape
    y = torch.empty((B, Cb, (H - 1) // stride + 1, (W - 1) // stride + 1, 8), dtype=torch.bfloat16, device=x.device)
    check(lib().rsis_blk_subsample2d(ptr(x), ptr(y), B, Cb * 8, H, W, int(stride), stream()), "rsis_blk_subsample2d")
    return y


def blk_upscatter(dy, H, W, stride):
    _blk_ok(dy)
    B, Cb, Ho, Wo, _ = dy.shape
    assert Ho == (H - 1) // stride + 1 and Wo == (W - 1) // stride + 1
    dx = torch.empty((B, Cb, H, W, 8), dtype=torch.bfloat16, device=dy.device)
    check(lib().rsis_blk_upscatter2d(ptr(dy), ptr(dx), B, Cb * 8, H, W, int(stride), stream()), "rsis_blk_upscatter2d")
    return dx


DTYPE_BF16_BLK = 2      # rsis_conv2d_wgrad / rsis_wgrad_job.dtype: dy and x are blk tensors


def blk_conv_wgrad(dy, x, dW, ks):
    """dW[Cout][Cin][ks][ks] += the weight gradient of the stride-1 'same' conv from blk dy / x (fp32 accumulation and output)"""
    _blk_ok(dy, x)
    B, Cbo, H, W, _ = dy.shape
    Cin = x.shape[1] * 8
    assert tuple(x.shape[2:4]) == (H, W) and tuple(dW.shape) == (Cbo * 8, Cin, ks, ks) and dW.dtype == torch.float32 and dW.is_contiguous()
    check(lib().rsis_conv2d_wgrad(ptr(dy), ptr(x), ptr(dW), B, Cin, H, W, Cbo * 8, H, W, ks, 1, ks // 2, Cin, 0, 0, DTYPE_BF16_BLK, stream()),
          "rsis_conv2d_wgrad(blk)")
    return dW


# ---------------------------------------------------------------------------------------------------------------------------
# the recurrent decoder on blk tensors (csrc/conv_blk_dec.hip, blk_dec.hip): raw batched ops, no autograd (rsis_amd/decoder_seq.py)
# ---------------------------------------------------------------------------------------------------------------------------
def blk_conv_job(srcs, wp, cout, cpack=0, bias=None, addend=None, dsts=None, hid=0, c_prev=None, c_out=None, h_out=None, act_out=None,
                 side_key=None, tile=0, shape=None):
    """one job of rsis_blk_conv3x3_batch (include/rsis_hip.h: rsis_blk_conv_job).  srcs: blk tensors [B][C/8][H][W][8]; plain epilogue:
    dsts = list of <= 2 blk outputs; LSTM epilogue: hid > 0 with c_prev / c_out (fp32 NCHW), h_out / act_out (blk), side_key (int64).
    shape = (B, H, W) when there is no source (gates = addend only).  Returns (struct, tensors it points to)."""
    _blk_ok(*srcs)
    j = _lib.BlkConvJob()
    j.nsrc = len(srcs)
    for k, s in enumerate(srcs):
        j.src[k], j.Csrc[k] = s.data_ptr(), s.shape[1] * 8
    if srcs:
        B, _cb, H, W, _ = srcs[0].shape
    else:
        B, H, W = shape
    j.B, j.H, j.W, j.Wp, j.Cout, j.Cpack = B, H, W, wp.data_ptr(), int(cout), int(cpack)
    j.bias = bias.data_ptr() if bias is not None else None
    j.addend = addend.data_ptr() if addend is not None else None
    j.hid, j.tile = int(hid), int(tile)
    if hid > 0:
        j.c_prev = c_prev.data_ptr() if c_prev is not None else None
        j.c_out, j.h_out = c_out.data_ptr(), h_out.data_ptr()
        j.act_out = act_out.data_ptr() if act_out is not None else None
        j.side_key = side_key.data_ptr() if side_key is not None else None
    else:
        _blk_ok(*dsts)
        j.ndst = len(dsts)
        for k, d in enumerate(dsts):
            j.dst[k], j.Cdst[k] = d.data_ptr(), d.shape[1] * 8
    return j, (srcs, wp, bias, addend, dsts, c_prev, c_out, h_out, act_out, side_key)


def blk_conv3x3_batch(jobs):
    """jobs: list of blk_conv_job results -- independent convs in grouped launches"""
    arr = (_lib.BlkConvJob * len(jobs))(*[j for j, _keep in jobs])
    check(lib().rsis_blk_conv3x3_batch(arr, len(jobs), stream()), "rsis_blk_conv3x3_batch")


def blk_resize_job(src, dst, dpool=None, arg=None, backward=False, scale=None):
    """forward: src = x [B][C/8][Hi][Wi][8] -> dst = y [B][C/8][Ho][Wo][8]; backward: src = dy (Ho x Wo) -> dst = dx (Hi x Wi), + dpool / arg.
    scale ([B][C] fp32): the job of the scaled entry points (the result's channel planes multiplied by it); all jobs of a batch alike"""
    _blk_ok(src, dst)
    j = _lib.BlkResizeJob() if scale is None else _lib.BlkResizeScaledJob()
    if scale is not None:
        j.scale = scale.data_ptr()
    small, big = (dst, src) if backward else (src, dst)
    j.src, j.dst = src.data_ptr(), dst.data_ptr()
    j.dpool = dpool.data_ptr() if dpool is not None else None
    j.arg = arg.data_ptr() if arg is not None else None
    j.B, j.C, j.Hi, j.Wi, j.Ho, j.Wo = small.shape[0], small.shape[1] * 8, small.shape[2], small.shape[3], big.shape[2], big.shape[3]
    return j, (src, dst, dpool, arg, scale)


def _blk_resize_batch(jobs, name):
    kind = type(jobs[0][0])
    assert all(type(j) is kind for j, _keep in jobs)
    if kind is _lib.BlkResizeScaledJob:
        name = name.replace("_batch", "_scaled_batch")
    arr = (kind * len(jobs))(*[j for j, _keep in jobs])
    check(getattr(lib(), name)(arr, len(jobs), stream()), name)


def blk_upsample_fwd_batch(jobs):
    _blk_resize_batch(jobs, "rsis_blk_upsample_fwd_batch")


def blk_upsample_bwd_batch(jobs):
    _blk_resize_batch(jobs, "rsis_blk_upsample_bwd_batch")


def blk_resize_mul_job(src, dst, mul):
    """y = resize(x) * mul (`-skip_mode mul`): src = x [B][C/8][Hi][Wi][8] -> dst = y [B][C/8][Ho][Wo][8], mul a blk tensor of y's shape"""
    _blk_ok(src, dst, mul)
    if mul.shape != dst.shape:
        raise ValueError("blk_resize_mul_job: the multiplier has the result's shape")
    j = _lib.BlkResizeMulJob()
    j.src, j.dst, j.mul = src.data_ptr(), dst.data_ptr(), mul.data_ptr()
    j.B, j.C, j.Hi, j.Wi, j.Ho, j.Wo = src.shape[0], src.shape[1] * 8, src.shape[2], src.shape[3], dst.shape[2], dst.shape[3]
    return j, (src, dst, mul)


def blk_upsample_mul_fwd_batch(jobs):
    arr = (_lib.BlkResizeMulJob * len(jobs))(*[j for j, _keep in jobs])
    check(lib().rsis_blk_upsample_mul_fwd_batch(arr, len(jobs), stream()), "rsis_blk_upsample_mul_fwd_batch")


def blk_mul_prep_job(dy, x, m, dm, accumulate):
    """backward preparation of y = resize(x) * m: dm (fp32 NCHW [B][C][Ho][Wo]) = dy * u, or fmaf(dy, u, dm) with accumulate, u = resize(x)
    rounded to bf16; then dy <- dy * m in place (include/rsis_hip.h: rsis_blk_mul_prep_job)"""
    _blk_ok(dy, x, m)
    B, Cb, Ho, Wo, _ = dy.shape
    if m.shape != dy.shape or dm.dtype != torch.float32 or tuple(dm.shape) != (B, Cb * 8, Ho, Wo) or not dm.is_contiguous() or x.shape[:2] != dy.shape[:2]:
        raise ValueError("blk_mul_prep_job: m has dy's shape, dm is its fp32 NCHW twin, x has dy's planes")
    j = _lib.BlkMulPrepJob()
    j.dy, j.x, j.m, j.dm = dy.data_ptr(), x.data_ptr(), m.data_ptr(), dm.data_ptr()
    j.B, j.C, j.Hi, j.Wi, j.Ho, j.Wo, j.accumulate = B, Cb * 8, x.shape[2], x.shape[3], Ho, Wo, int(bool(accumulate))
    return j, (dy, x, m, dm)


def blk_upsample_mul_bwd_prep_batch(jobs):
    arr = (_lib.BlkMulPrepJob * len(jobs))(*[j for j, _keep in jobs])
    check(lib().rsis_blk_upsample_mul_bwd_prep_batch(arr, len(jobs), stream()), "rsis_blk_upsample_mul_bwd_prep_batch")


def blk_lstm_bwd_job(dh, dh2, dc_next, act, c_prev, c, da, dc_prev):
    _blk_ok(dh, dh2, act, da)
    j = _lib.BlkLstmBwdJob()
    for k, t in (("dh", dh), ("dh2", dh2), ("dc_next", dc_next), ("act", act), ("c_prev", c_prev), ("c", c), ("da", da), ("dc_prev", dc_prev)):
        setattr(j, k, t.data_ptr() if t is not None else None)
    j.B, j.hid, j.HW = dh.shape[0], dh.shape[1] * 8, dh.shape[2] * dh.shape[3]
    return j, (dh, dh2, dc_next, act, c_prev, c, da, dc_prev)


def blk_lstm_bwd_batch(jobs):
    arr = (_lib.BlkLstmBwdJob * len(jobs))(*[j for j, _keep in jobs])
    check(lib().rsis_blk_lstm_bwd_batch(arr, len(jobs), stream()), "rsis_blk_lstm_bwd_batch")
