"""Shared test helpers (oracle = CPU checker; the product runs on cuda:0 through librsis_hip.so)."""
import argparse
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mk_args(hidden_size=128, num_classes=21, maxseqlen=10, **kw):
    a = argparse.Namespace(use_gpu=True, base_model="resnet101", hidden_size=hidden_size, kernel_size=3,
                           num_classes=num_classes, dropout=0.0, dropout_stop=0.0, dropout_cls=0.0, skip_mode="concat",
                           maxseqlen=maxseqlen, gt_maxseqlen=20, iou_weight=1.0, class_weight=0.1, stop_weight=0.5,
                           stop_balance_weight=0.5, use_class_loss=True, use_stop_loss=True, curriculum_learning=False,
                           update_encoder=True)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def assert_close(what, got, want, atol, rtol=0.0):
    got = torch.as_tensor(got).detach().double().cpu()
    want = torch.as_tensor(np.asarray(want) if not torch.is_tensor(want) else want).detach().double().cpu()
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(want.shape))
    if got.numel() == 0:
        return
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    if os.environ.get("RSIS_TEST_MARGINS"):        # margin survey: worst err / tol of every comparison, one line per call
        with open(os.environ["RSIS_TEST_MARGINS"], "a") as f:
            ratio = float((err / tol.clamp_min(1e-300)).max()) if tol.numel() else 0.0
            f.write("%.4f\t%s\t%s\n" % (ratio, os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], what))
    bad = err > tol
    if bad.any() or torch.isnan(got).any():
        i = int(torch.argmax(err - tol))
        idx = np.unravel_index(i, got.shape) if got.dim() else ()
        raise AssertionError("%s: max abs err %.3e (tol %.1e + %.1e*|ref|) at %s: got %.6g want %.6g; %d/%d bad; |ref|max %.3g"
                             % (what, float(err.max()), atol, rtol, idx, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]),
                                int(bad.sum()), got.numel(), float(want.abs().max())))


def same_matching(what, assignment, class_perm, ref_scores, ref_class_perm, tie=1e-5):
    """The matching of reference train.py:137 is an arg-min over assignments: it is defined only up to ties of the cost matrix.  With
    random weights the predicted masks of an image barely change over the timesteps, so the columns of its cost matrix are almost equal
    and the optimum beats the next assignment by ~1e-6 (BASELINE configs[1] on the synthetic batch: every image) -- less than two fp32
    evaluations of the soft IoU differ by.  So: the product's permuted class targets must EQUAL the reference's (returns True), or
    its assignment must be as good as the optimum UNDER THE REFERENCE'S OWN COSTS to within `tie` for every image (returns False: the
    caller then compares what depends on the assignment against the reference evaluated under that assignment)."""
    from scipy.optimize import linear_sum_assignment
    got = torch.as_tensor(class_perm).cpu().numpy()
    want = np.asarray(ref_class_perm)
    if got.shape == want.shape and (got == want).all():
        return True
    S = np.asarray(ref_scores, dtype=np.float64)
    A = torch.as_tensor(assignment).cpu().numpy()
    T = S.shape[2]
    for b in range(S.shape[0]):
        cols = A[b, :T]
        assert len(set(cols.tolist())) == T, "%s: image %d: not an assignment: %s" % (what, b, cols)
        ri, ci = linear_sum_assignment(S[b])
        best, mine = S[b][ri, ci].sum(), S[b][cols, np.arange(T)].sum()
        assert mine <= best + tie, "%s: image %d: assignment %s costs %.7f under the reference's scores, the optimum %.7f" % (what, b, cols, mine, best)
    return False


def sub_idx(n, cap=4096):
    """the deterministic sub-sample oracle/make_golden.py stores of a flat gradient / parameter vector"""
    return slice(0, n, max(1, n // cap))


# ---- host models of the fp32 summation order of the direct 3x3 kernels (test_gpu_infer_paths.py, test_infer_paths_host.py)
CK, ACC_FLUSH = 8, 4          # RSIS_CK, RSIS_ACC_FLUSH of csrc/conv3x3_direct.hip


def f32_normal(seed, shape, scale=1.0):
    return np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32)


def to_tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def max_err(a, ref):
    """max |a - ref| in float64; a: a tensor on any device or a numpy array, ref: a float64 tensor on the host"""
    a = a.detach().double().cpu() if torch.is_tensor(a) else to_tensor(a).double()
    return float((a - ref).abs().max())


def host_sums(xs, w, b):
    """3x3 / stride 1 / pad 1 conv of the channel concat of xs (float32 arrays) formed with fp32 products and fp32 additions in the two
    summation orders; returns (chain, segmented), float32 (B, Cout, H, W).  `chain`: one running sum, sources in order, channels
    ascending, taps row-major.  `segmented`: the same order, the running sum moved to a second fp32 total every ACC_FLUSH chunks of CK
    channels, chunks counted on across the sources as the kernel counts them.  The bias is added last, as the kernels' epilogues add it."""
    B, _, H, W = xs[0].shape
    Cout = w.shape[0]
    chain = np.zeros((B, Cout, H, W), np.float32)
    acc, tot = np.zeros_like(chain), np.zeros_like(chain)
    chunk, c_off = 0, 0
    for x in xs:
        xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
        for c in range(x.shape[1]):
            if c % CK == 0:                      # chunk number `chunk` (counted from 0 across the sources) begins
                if chunk > 0 and chunk % ACC_FLUSH == 0:
                    tot += acc
                    acc[:] = 0
                chunk += 1
            for r in range(3):
                for s in range(3):
                    term = w[None, :, c_off + c, r, s, None, None] * xp[:, None, c, r:r + H, s:s + W]
                    chain += term
                    acc += term
        c_off += x.shape[1]
    seg = tot + acc
    if b is not None:
        chain, seg = chain + b[None, :, None, None], seg + b[None, :, None, None]
    assert chain.dtype == np.float32 and seg.dtype == np.float32
    return chain, seg


def _sums_padded(xps, w, Ho, Wo, stride):
    """the loop of host_sums for any square kernel and stride over sources that already carry their padding: out[b, co, y, x] = sum over
    (source, channel, r, s) of w[co, c, r, s] * xp[b, c, y * stride + r, x * stride + s]; returns (chain, segmented) without a bias"""
    B, Cout, ks = xps[0].shape[0], w.shape[0], w.shape[2]
    chain = np.zeros((B, Cout, Ho, Wo), np.float32)
    acc, tot = np.zeros_like(chain), np.zeros_like(chain)
    chunk, c_off = 0, 0
    for xp in xps:
        for c in range(xp.shape[1]):
            if c % CK == 0:
                if chunk > 0 and chunk % ACC_FLUSH == 0:
                    tot += acc
                    acc[:] = 0
                chunk += 1
            for r in range(ks):
                for s in range(ks):
                    term = w[None, :, c_off + c, r, s, None, None] * xp[:, None, c, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]
                    chain += term
                    acc += term
        c_off += xp.shape[1]
    seg = tot + acc
    assert chain.dtype == np.float32 and seg.dtype == np.float32
    return chain, seg


def host_sums_conv(xs, w, b, stride=1, pad=1):
    """host_sums for any square kernel, stride and padding (3x3 / stride 1 / pad 1: the same bits as host_sums).  The order is the one the
    implicit-GEMM kernels walk as well: k = (channel over the concat, r, s) ascending."""
    ks = w.shape[2]
    H, W = xs[0].shape[2:]
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    chain, seg = _sums_padded([np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad))) for x in xs], w, Ho, Wo, stride)
    if b is not None:
        chain, seg = chain + b[None, :, None, None], seg + b[None, :, None, None]
    return chain, seg


def host_sums_dgrad(dy, w, stride, pad, Hx, Wx):
    """the data gradient dx (B, Cin, Hx, Wx) of a conv with weight w (Cout, Cin, ks, ks) as the kernels form it: a stride-1 conv that
    gathers from dy (B, Cout, Hy, Wx) with the ROTATED, TRANSPOSED weights wT[ci, co, r', s'] = w[co, ci, ks-1-r', ks-1-s'], the reduction
    walked over the Cout rows of dy ascending (chunks of CK of THEM, as the direct kernel counts) and the taps row-major.  A strided
    conv's gradient gathers from dy spread out with zeros (dy[yo, xo] at pixel (yo * stride, xo * stride)): the products with those
    zeros are exact zeros and leave an fp32 running sum unchanged, so the order of the non-zero terms is the kernels' (the parity-class
    kernel and the strided gathers skip exactly those terms).  Returns (chain, segmented), float32."""
    B, Cout, Hy, Wy = dy.shape
    ks = w.shape[2]
    lo = ks - 1 - pad
    up = np.zeros((B, Cout, Hx + ks - 1, Wx + ks - 1), np.float32)
    ny, nx = min(Hy, (Hx + ks - 2 - lo) // stride + 1), min(Wy, (Wx + ks - 2 - lo) // stride + 1)
    up[:, :, lo:lo + (ny - 1) * stride + 1:stride, lo:lo + (nx - 1) * stride + 1:stride] = dy[:, :, :ny, :nx]
    wT = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
    return _sums_padded([up], wT, Hx, Wx, 1)


# ---- the ConvLSTM cell in float64 and the bar of its gate pre-activations (test_gpu_infer_paths.py, test_gpu_train_paths.py)
def cell64(w, b, xs, state, pad=1):
    """clstm.py:43-58 in float64 (test_gpu_bf16._oracle_cell_rounded without the rounding); returns (h, c, gate pre-activations, in the
    reference's row order [i | f | o | g])"""
    import torch.nn.functional as F
    srcs = [to_tensor(x).double() for x in xs] + ([state[0].double()] if state is not None else [])
    cin = sum(s.shape[1] for s in srcs)
    gates = F.conv2d(torch.cat(srcs, 1), to_tensor(w).double()[:, :cin], to_tensor(b).double(), padding=pad)
    i, f, o, g = gates.chunk(4, 1)
    i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
    c = f * (state[1].double() if state is not None else 0.0) + i * g
    return o * torch.tanh(c), c, gates


def gate_bar(w, b, xs, state, gates64, m, model="segmented", pad=1):
    """e = m * err_host + 2e-7: the tight bar of the gate pre-activations of this call.  err_host: the host model (`segmented` for an
    inference call, `chain` for a training call below RSIS_FLUSH_MIN_CHUNKS chunks) of the gate conv over the sources the kernel walks."""
    srcs = list(xs) + ([state[0].float().numpy()] if state is not None else [])
    cin = sum(s.shape[1] for s in srcs)
    wc = np.ascontiguousarray(w[:, :cin])
    chain, seg = host_sums(srcs, wc, b) if (w.shape[2] == 3 and pad == 1) else host_sums_conv(srcs, wc, b, 1, pad)
    return m * max_err(seg if model == "segmented" else chain, gates64) + 2e-7


# ---- the fp32 ConvLSTM pointwise backward (test_gpu_decoder_bwd_ops.py, test_decoder_bwd_host.py): reference, bars, guarded buffers
LSTM_BWD_K = 24               # allowed error in units of 2^-24 * lstm_bwd_scales(..): see test_decoder_bwd_host.py for the derivation
LSTM_BWD_OUTS = ("da_i", "da_f", "da_o", "da_g", "dc_prev")


def lstm_bwd_inputs(seed, B, hid, HW, c_scale=1.0):
    """fp32 operands of one cell's pointwise backward: act (B, 4 hid, HW) in gate-interleaved rows 4 j + gate (i, f, o sigmoid, g tanh of
    N(0, 2) pre-activations, so saturated gates occur), c / c_prev N(0, c_scale), dh / dh2 / dc_next N(0, 1)"""
    rs = np.random.default_rng(seed)
    pre = rs.normal(0, 2, (B, hid, 4, HW))
    act = np.concatenate([1.0 / (1.0 + np.exp(-pre[:, :, :3])), np.tanh(pre[:, :, 3:])], 2).astype(np.float32).reshape(B, 4 * hid, HW)
    n = lambda s: rs.normal(0, s, (B, hid, HW)).astype(np.float32)
    return dict(act=act, c=n(c_scale), c_prev=n(c_scale), dh=n(1), dh2=n(1), dc_next=n(1))


def _lstm_bwd_terms(q, dt):
    """the operands of pointwise.hip's header formulas in dtype dt; an absent operand (None) is 0"""
    B, hid4, HW = q["act"].shape
    a = q["act"].astype(dt).reshape(B, hid4 // 4, 4, HW)
    z = np.zeros((B, hid4 // 4, HW), dt)
    get = lambda k: q[k].astype(dt) if q.get(k) is not None else z
    return a[:, :, 0], a[:, :, 1], a[:, :, 2], a[:, :, 3], q["c"].astype(dt), get("c_prev"), get("dh"), get("dh2"), get("dc_next")


def lstm_bwd_eval(q, dt=np.float64):
    """do = dh tanh(c); dc = dc_next + dh o (1 - tanh(c)^2); da_i = dc g i (1 - i), da_f = dc c_prev f (1 - f), da_o = do o (1 - o),
    da_g = dc i (1 - g^2), dc_prev = dc f  (dh = dh + dh2), every operation in dtype dt: float64 is the reference, float32 the host
    model of the kernels' arithmetic.  Returns {name: (B, hid, HW)} for LSTM_BWD_OUTS."""
    i, f, o, g, c, cp, dh, dh2, dn = _lstm_bwd_terms(q, dt)
    one = dt(1)
    tc = np.tanh(c)
    dhv = dh + dh2
    dcv = dhv * o * (one - tc * tc) + dn
    out = dict(da_i=dcv * g * i * (one - i), da_f=dcv * cp * f * (one - f), da_o=dhv * tc * o * (one - o), da_g=dcv * i * (one - g * g),
               dc_prev=dcv * f)
    assert all(v.dtype == dt for v in out.values())
    return out


def lstm_bwd_scales(q):
    """per-element magnitudes that one fp32 rounding is measured against (float64), M = (|dh| + |dh2|) o + |dc_next|: cancellation in dc
    and in 1 - g^2 is charged to the terms that cancel, not hidden behind max|ref|.  The 1/8 of da_g admits the one ABSOLUTE rounding
    of g^2 next to 1."""
    i, f, o, g, c, cp, dh, dh2, dn = _lstm_bwd_terms(q, np.float64)
    adh = np.abs(dh) + np.abs(dh2)
    M = adh * o + np.abs(dn)
    return dict(da_i=M * np.abs(g * i * (1 - i)), da_f=M * np.abs(cp * f * (1 - f)), da_o=adh * np.abs(np.tanh(c)) * o * (1 - o),
                da_g=M * i * ((1 - g * g) + 0.125), dc_prev=M * f)


def lstm_bwd_ratios(got, q):
    """{name: worst |got - float64 reference| / (2^-24 * scale)} over the outputs present in `got` ({name: (B, hid, HW) array});
    where the scale is 0 the output must be exactly the reference (inf otherwise)"""
    ref, sc = lstm_bwd_eval(q), lstm_bwd_scales(q)
    worst = {}
    for k, v in got.items():
        v = np.asarray(v, np.float64)
        assert v.shape == ref[k].shape, "%s: shape %s vs %s" % (k, v.shape, ref[k].shape)
        if not np.isfinite(v).all():
            worst[k] = float("inf")
            continue
        err, s = np.abs(v - ref[k]), sc[k] * 2.0 ** -24
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(s > 0, err / s, np.where(err > 0, np.inf, 0.0))
        worst[k] = float(r.max())
    return worst


def split_da(da):
    """(B, 4 hid, HW) gate-interleaved rows -> {da_i, da_f, da_o, da_g: (B, hid, HW)}"""
    da = np.asarray(da)
    B, hid4, HW = da.shape
    v = da.reshape(B, hid4 // 4, 4, HW)
    return dict(da_i=v[:, :, 0], da_f=v[:, :, 1], da_o=v[:, :, 2], da_g=v[:, :, 3])


GUARD, SENTINEL = 64, -12345.5


class Guarded(object):
    """an output tensor as a view into one larger allocation with GUARD floats of SENTINEL on each side: .t is the view (filled with
    SENTINEL, or with `init`), .check() asserts that both guard zones still hold the sentinel -- writes outside the tensor but inside
    the allocation are seen, nothing is provoked.  offset: extra floats in front (1: a view that is not 16-byte aligned)."""

    def __init__(self, shape, device="cuda", init=None, offset=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD + offset,), SENTINEL, dtype=torch.float32, device=device)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(init))

    def check(self, what="output"):
        lo, hi = self.buf[:self.lo], self.buf[self.hi:]
        assert hi.numel() == GUARD
        assert bool((lo == SENTINEL).all()), "%s: the guard zone in FRONT of the tensor was written" % what
        assert bool((hi == SENTINEL).all()), "%s: the guard zone BEHIND the tensor was written" % what

    def untouched(self):
        return bool((self.t == SENTINEL).all())
