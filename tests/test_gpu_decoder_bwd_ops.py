"""The backward entry points of the fp32 sequence decoder (rsis_amd/decoder_seq.py), op by op through the C ABI: rsis_conv_out_seq_fwd /
_dgrad / _wgrad (conv_c1.hip with seqT > 1), rsis_convlstm_bwd_gates and _batch, rsis_sum_leading, rsis_bias_grad.  Every reference is
float64 on the host (or the exact comparison named at the test).  Two data regimes:

  * EXACT (coverage and indexing): inputs are integers in -3..3 stored as fp32, accumulated outputs are prefilled with non-zero integers.
    Every product and every partial sum is an integer below 2^24 (asserted on the reference: sum of |terms| < 2^24), so fp32 arithmetic
    is exact in ANY order -- fma, shuffles and atomics included -- and the kernels must EQUAL the float64 reference, in the default and
    in the deterministic mode.  A skipped or doubly visited tile, a wrong (t, b) image pairing or a wrong gate row fails at zero tolerance.
  * NORMAL (rounding): seeded N(0, 1) data, conv weights scaled by 1 / sqrt(9 Cin); bars per op:
      conv fwd / dgrad     2e-6 sqrt(9 Cin) + 1e-6 (the bar of test_gpu_wino.py);
      conv wgrad / db      1e-4 max(1, max|ref|) (the bar of test_gpu_ops.py; coverage rests on the exact regime);
      LSTM backward        per element LSTM_BWD_K = 24 units of 2^-24 * helpers.lstm_bwd_scales(..) (derivation: test_decoder_bwd_host.py);
      bias gradient        deterministic mode: 4 * 2^-24 (|prefill| + |ref|) -- the sum is formed in double, one cast and one add round;
      sum over timesteps   bit-equal to the fp32 loop acc = x[0]; acc = acc + x[t], t ascending (IEEE additions in a fixed order).

Every output is a view into a larger allocation with 64 sentinel floats on each side (helpers.Guarded), checked after the call.
Measured figures and the mutation runs that show this file can fail: NOTES.md (77)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import (LSTM_BWD_K, Guarded, assert_close, f32_normal as _rng, lstm_bwd_inputs, lstm_bwd_ratios, max_err as _err, split_da,
                     to_tensor as _t)

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 3           # RSIS_ERR_UNSUPPORTED of csrc/common.h
EXACT_LIMIT = 2.0 ** 24


@pytest.fixture(params=["default", "deterministic"])
def mode(request):
    from rsis_amd import ops
    prev = ops.set_deterministic(request.param == "deterministic")
    yield request.param
    ops.set_deterministic(prev)


@pytest.fixture
def deterministic():
    from rsis_amd import ops
    prev = ops.set_deterministic(True)
    yield
    ops.set_deterministic(prev)


def _ints(seed, shape, lo=-3, hi=3, nonzero=False):
    v = np.random.default_rng(seed).integers(lo, hi + 1, shape)
    if nonzero:
        v = np.where(v == 0, hi, v)
    return v.astype(np.float32)


# ---------------------------------------------------------------- rsis_conv_out_seq_*
SEQ_CASES = [
    # (T, B, Cin, H, W)
    (3, 2, 8, 12, 64),       # 64-wide tiles, partial tile rows
    (2, 3, 16, 20, 72),      # 128-wide tile on a 72-wide image, several channel passes
    (3, 2, 4, 9, 160),       # 256-wide tile on a 160-wide image, two tile rows with the second partial
    (1, 4, 8, 16, 16),       # \ the two cases where the [t][b] <-> [b][t] map is the identity
    (5, 1, 8, 16, 16),       # /
    (3, 5, 16, 80, 64),      # 75 tiles x 8 channel pairs = 600 > 512: the persistent weight-gradient loop, in both modes
]
SEQ_BIG = (3, 2, 4, 420, 420)     # 1 058 400 pixels > 4096 x 256: the grid-stride loop of the data gradient (exact regime only)
_SEQ = {}


def _seq_id(c):
    return "T%d_B%d_C%d_%dx%d" % c


def _wgrad64(dy_tb, x, absolute=False):
    """dW[ci][r][s] = sum over images and pixels of dy * (zero-padded x shifted by the tap), float64; dy_tb (N, H, W), x (N, Cin, H, W).
    absolute: the sum of |terms| instead (a bound on every partial sum in any order)."""
    N, Cin, H, W = x.shape
    d, xp = dy_tb.double(), F.pad(x.double(), (1, 1, 1, 1))
    if absolute:
        d, xp = d.abs(), xp.abs()
    out = torch.empty(Cin, 3, 3, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            out[:, r, s] = (xp[:, :, r:r + H, s:s + W] * d[:, None]).sum((0, 2, 3))
    return out.view(1, Cin, 3, 3)


def _seq(case, regime, need=("fwd", "dgrad", "wgrad")):
    """host inputs and float64 references of one case, computed once and shared (never modified): x [T][B][Cin][H][W], y and dy
    [B][T][H W] -- image t * B + b of the former pairs with image b * T + t of the latter"""
    key = (case, regime)
    if key not in _SEQ:
        T, B, Cin, H, W = case
        seed = 1000 + 7 * sum(case)
        if regime == "exact":
            x, dy = _ints(seed, (T, B, Cin, H, W)), _ints(seed + 1, (B, T, H * W))
            w, b = _ints(seed + 2, (1, Cin, 3, 3), nonzero=True), _ints(seed + 3, (1,), nonzero=True)
            dW0, db0 = _ints(seed + 4, (1, Cin, 3, 3), -9, 9, nonzero=True), _ints(seed + 5, (1,), 5, 9)
        else:
            x, dy = _rng(seed, (T, B, Cin, H, W)), _rng(seed + 1, (B, T, H * W))
            w, b = _rng(seed + 2, (1, Cin, 3, 3), 1.0 / np.sqrt(9 * Cin)), _rng(seed + 3, (1,)) + np.float32(0.5)
            dW0, db0 = _rng(seed + 4, (1, Cin, 3, 3)), _rng(seed + 5, (1,))
        r = dict(x=_t(x), dy=_t(dy), w=_t(w), b=_t(b), dW0=_t(dW0), db0=_t(db0))
        x4 = r["x"].view(T * B, Cin, H, W)
        dy_tb = r["dy"].view(B, T, H, W).transpose(0, 1).reshape(T * B, H, W)             # [t][b] order, as x
        if "fwd" in need:
            r["y"] = F.conv2d(x4.double(), r["w"].double(), r["b"].double(), padding=1).view(T, B, H * W).transpose(0, 1).contiguous()
        if "dgrad" in need:
            r["dx"] = F.conv_transpose2d(dy_tb[:, None].double(), r["w"].double(), padding=1).view(T, B, Cin, H, W)
        if "wgrad" in need:
            r["dW"] = r["dW0"].double() + _wgrad64(dy_tb, x4)
            r["db"] = r["db0"].double() + r["dy"].double().sum()
        if regime == "exact":                     # what makes "equal in any order" true: every partial sum is an integer below 2^24
            bound = float(r["w"].abs().sum()) * 3 + float(r["b"].abs())
            if "wgrad" in need:
                bound = max(bound, float((r["dW0"].abs().double() + _wgrad64(dy_tb, x4, True)).max()), float(r["db0"].abs() + r["dy"].abs().double().sum()))
            assert bound < EXACT_LIMIT, "exact regime: partial sums up to %g" % bound
        _SEQ[key] = r
    return _SEQ[key]


def _packs(w, Cin):
    from rsis_amd import ops
    pack = ops.PackedConv(3, [Cin])
    wd = w.cuda()
    return pack, wd, pack.fwd(wd), pack.dgrad(wd)


def _seq_fwd(r, case, wp):
    from rsis_amd._lib import check, lib, ptr, stream
    T, B, Cin, H, W = case
    xd, bd = r["x"].cuda(), r["b"].cuda()
    y = Guarded((B, T, H * W))
    check(lib().rsis_conv_out_seq_fwd(ptr(xd), ptr(wp), ptr(bd), ptr(y.t), T, B, Cin, H, W, stream()), "rsis_conv_out_seq_fwd")
    torch.cuda.synchronize()
    y.check("y")
    return y.t, xd, bd


def _seq_dgrad(r, case, wdp):
    from rsis_amd._lib import check, lib, ptr, stream
    T, B, Cin, H, W = case
    dyd = r["dy"].cuda()
    dx = Guarded((T, B, Cin, H, W))
    check(lib().rsis_conv_out_seq_dgrad(ptr(dyd), ptr(wdp), ptr(dx.t), T, B, Cin, H, W, stream()), "rsis_conv_out_seq_dgrad")
    torch.cuda.synchronize()
    dx.check("dx")
    return dx.t, dyd


def _seq_wgrad(r, case):
    from rsis_amd._lib import check, lib, ptr, stream
    T, B, Cin, H, W = case
    xd, dyd = r["x"].cuda(), r["dy"].cuda()
    dW, db = Guarded((1, Cin, 3, 3), init=r["dW0"]), Guarded((1,), init=r["db0"])
    check(lib().rsis_conv_out_seq_wgrad(ptr(dyd), ptr(xd), ptr(dW.t), ptr(db.t), T, B, Cin, H, W, stream()), "rsis_conv_out_seq_wgrad")
    torch.cuda.synchronize()
    dW.check("dW")
    db.check("db")
    return dW.t, db.t


def _equal64(what, got, ref):
    got = got.detach().double().cpu()
    bad = got != ref
    assert not bool(bad.any()), "%s: %d of %d elements differ from the float64 reference in the exact regime (worst %g)" % (
        what, int(bad.sum()), got.numel(), float((got - ref).abs().max()))


@pytest.mark.parametrize("case", SEQ_CASES, ids=_seq_id)
def test_conv_out_seq_fwd_exact(case):
    r = _seq(case, "exact")
    _pack, _w, wp, _wd = _packs(r["w"], case[2])
    y, _x, _b = _seq_fwd(r, case, wp)
    _equal64("y", y, r["y"])


@pytest.mark.parametrize("case", SEQ_CASES + [SEQ_BIG], ids=_seq_id)
def test_conv_out_seq_dgrad_exact(case):
    r = _seq(case, "exact", need=("dgrad",) if case == SEQ_BIG else ("fwd", "dgrad", "wgrad"))
    _pack, _w, _wp, wdp = _packs(r["w"], case[2])
    dx, _dy = _seq_dgrad(r, case, wdp)
    _equal64("dx", dx, r["dx"])


@pytest.mark.parametrize("case", SEQ_CASES, ids=_seq_id)
def test_conv_out_seq_wgrad_exact(case, mode):
    r = _seq(case, "exact")
    dW, db = _seq_wgrad(r, case)
    _equal64("dW (%s mode)" % mode, dW, r["dW"])
    _equal64("db (%s mode)" % mode, db, r["db"])


@pytest.mark.parametrize("case", SEQ_CASES, ids=_seq_id)
def test_conv_out_seq_fwd_normal_and_per_step(case):
    """within the fp32 bar of float64, and image (t, b) bit-equal to rsis_conv2d_fwd on step t's input alone ("same kernels and
    per-image arithmetic", include/rsis_hip.h)"""
    from rsis_amd._lib import check, int_array, lib, ptr, ptr_array, stream
    T, B, Cin, H, W = case
    r = _seq(case, "normal")
    pack, _w, wp, _wd = _packs(r["w"], Cin)
    y, xd, bd = _seq_fwd(r, case, wp)
    print("\nBWD-OPS conv_out_seq_fwd %s: err %.3e (bar %.3e)" % (_seq_id(case), _err(y, r["y"]), 2e-6 * np.sqrt(9 * Cin) + 1e-6))
    assert_close("y", y, r["y"], 2e-6 * np.sqrt(9 * Cin) + 1e-6)
    for t in range(T):
        one = Guarded((B, 1, H, W))
        check(lib().rsis_conv2d_fwd(ptr_array([xd[t]]), int_array([Cin]), 1, B, H, W, ptr(wp), 1, 3, 1, 1, ptr(bd), None, ptr(one.t), H, W, 0,
                                    pack.dtype, stream()), "rsis_conv2d_fwd")
        torch.cuda.synchronize()
        one.check("single-step y")
        assert torch.equal(y[:, t], one.t.view(B, H * W)), "step %d: the sequence forward differs from rsis_conv2d_fwd on that step" % t


@pytest.mark.parametrize("case", SEQ_CASES, ids=_seq_id)
def test_conv_out_seq_dgrad_normal_and_per_step(case):
    from rsis_amd._lib import check, int_array, lib, ptr, ptr_array, stream
    T, B, Cin, H, W = case
    r = _seq(case, "normal")
    pack, _w, _wp, wdp = _packs(r["w"], Cin)
    dx, dyd = _seq_dgrad(r, case, wdp)
    print("\nBWD-OPS conv_out_seq_dgrad %s: err %.3e (bar %.3e)" % (_seq_id(case), _err(dx, r["dx"]), 2e-6 * np.sqrt(9 * Cin) + 1e-6))
    assert_close("dx", dx, r["dx"], 2e-6 * np.sqrt(9 * Cin) + 1e-6)
    for t in range(T):
        one = Guarded((B, Cin, H, W))
        dy_t = dyd[:, t].contiguous()
        check(lib().rsis_conv2d_dgrad(ptr(dy_t), B, 1, H, W, ptr(wdp), Cin, 3, 1, 1, ptr_array([one.t]), int_array([Cin]), 1, H, W, None, 0,
                                      pack.dtype, stream()), "rsis_conv2d_dgrad")
        torch.cuda.synchronize()
        one.check("single-step dx")
        assert torch.equal(dx[t], one.t), "step %d: the sequence data gradient differs from rsis_conv2d_dgrad on that step" % t


@pytest.mark.parametrize("case", SEQ_CASES, ids=_seq_id)
def test_conv_out_seq_wgrad_normal(case, mode):
    r = _seq(case, "normal")
    dW, db = _seq_wgrad(r, case)
    bw, bb = 1e-4 * max(1.0, float(r["dW"].abs().max())), 1e-4 * max(1.0, float(r["db"].abs().max()))
    print("\nBWD-OPS conv_out_seq_wgrad %s, %s mode: err dW %.3e (bar %.3e, max|ref| %.3g)  err db %.3e (bar %.3e, |ref| %.3g)"
          % (_seq_id(case), mode, _err(dW, r["dW"]), bw, float(r["dW"].abs().max()), _err(db, r["db"]), bb, float(r["db"].abs().max())))
    assert_close("dW", dW, r["dW"], bw)
    assert_close("db", db, r["db"], bb)
    if mode == "deterministic":
        dW2, db2 = _seq_wgrad(r, case)
        assert torch.equal(dW, dW2) and torch.equal(db, db2), "deterministic mode: two calls from the same prefill must give the same bits"


@pytest.mark.parametrize("T,B,Cin,H,W", [(3, 2, 6, 12, 64), (3, 2, 8, 12, 18)], ids=["Cin6", "W18"])
def test_conv_out_seq_unsupported_shapes_write_nothing(T, B, Cin, H, W):
    from rsis_amd._lib import lib, ptr, stream
    L = lib()
    x, dy = _t(_rng(1, (T, B, Cin, H, W))).cuda(), _t(_rng(2, (B, T, H * W))).cuda()
    w, b = _t(_rng(3, (1, Cin, 3, 3))), _t(_rng(4, (1,))).cuda()
    _pack, _w, wp, wdp = _packs(w, Cin)
    y, dx, dW, db = Guarded((B, T, H * W)), Guarded((T, B, Cin, H, W)), Guarded((1, Cin, 3, 3)), Guarded((1,))
    assert L.rsis_conv_out_seq_fwd(ptr(x), ptr(wp), ptr(b), ptr(y.t), T, B, Cin, H, W, stream()) == ERR_UNSUPPORTED
    assert L.rsis_conv_out_seq_dgrad(ptr(dy), ptr(wdp), ptr(dx.t), T, B, Cin, H, W, stream()) == ERR_UNSUPPORTED
    assert L.rsis_conv_out_seq_wgrad(ptr(dy), ptr(x), ptr(dW.t), ptr(db.t), T, B, Cin, H, W, stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for name, g in (("y", y), ("dx", dx), ("dW", dW), ("db", db)):
        g.check(name)
        assert g.untouched(), "%s was written by a call that returned RSIS_ERR_UNSUPPORTED" % name


# ---------------------------------------------------------------- rsis_convlstm_bwd_gates / _batch
LSTM_SHAPES = [(2, 4, 5, 7), (2, 8, 8, 8), (3, 16, 9, 12), (1, 128, 4, 4), (2, 3, 6, 5)]      # (B, hid, H, W)
V4_SHAPES = [s for s in LSTM_SHAPES if (s[2] * s[3]) % 4 == 0]
FORMS = {"full": (), "t0": ("c_prev", "dc_prev"), "last": ("dh2", "dc_next")}                 # the operands that are NULL
_IN = ("dh", "dh2", "dc_next", "act", "c_prev", "c")


def _lstm_id(s):
    return "B%d_h%d_%dx%d" % s


def _job(shape, form, seed, c_scale, nonfinite=False):
    B, hid, H, W = shape
    q = lstm_bwd_inputs(seed, B, hid, H * W, c_scale)
    for k in FORMS[form]:
        if k in q:
            q[k] = None
    if nonfinite:
        flat = q["c"].reshape(-1)
        flat[[0, 1, 2, 3, 5, flat.size - 1]] = [np.inf, -np.inf, 1e30, -1e30, np.inf, -np.inf]
    q["shape"], q["form"] = shape, form
    return q


def _dev(q, misalign=None):
    """device copies of a job's operands (None stays None); `misalign` names one that becomes a view at a storage offset of 1 float"""
    d = {}
    for k in _IN:
        if q[k] is None:
            d[k] = None
        elif k == misalign:
            buf = torch.empty(q[k].size + 1, device="cuda")
            d[k] = buf[1:].view(*q[k].shape)
            d[k].copy_(_t(q[k]))
            assert d[k].data_ptr() % 16 == 4
        else:
            d[k] = _t(q[k]).cuda()
    return d


def _outputs(q, offset=0):
    B, hid, H, W = q["shape"]
    da = Guarded((B, 4 * hid, H * W), offset=offset)
    dcp = Guarded((B, hid, H * W)) if "dc_prev" not in FORMS[q["form"]] else None
    return da, dcp


def _check_job(what, q, da, dcp, record):
    torch.cuda.synchronize()
    da.check(what + " da")
    got = split_da(da.t.cpu().numpy())
    if dcp is not None:
        dcp.check(what + " dc_prev")
        got["dc_prev"] = dcp.t.cpu().numpy()
    assert all(np.isfinite(v).all() for v in got.values()), "%s: a non-finite output" % what
    worst = lstm_bwd_ratios(got, q)
    record.append(max(worst.values()))
    assert max(worst.values()) <= LSTM_BWD_K, "%s (%s, form %s): worst error in units of 2^-24 * scale %s > %d" % (
        what, _lstm_id(q["shape"]), q["form"], {k: round(v, 2) for k, v in worst.items()}, LSTM_BWD_K)


def _single(q, d, da, dcp, da_sum=None):
    from rsis_amd._lib import check, lib, ptr, stream
    B, hid, H, W = q["shape"]
    check(lib().rsis_convlstm_bwd_gates(ptr(d["dh"]), ptr(d["dh2"]), ptr(d["dc_next"]), ptr(d["act"]), ptr(d["c_prev"]), ptr(d["c"]), ptr(da.t),
                                        ptr(dcp.t) if dcp is not None else None, ptr(da_sum), B, hid, H * W, stream()), "rsis_convlstm_bwd_gates")


def _batch(jobs, misalign=None, da_offset=None):
    """one rsis_convlstm_bwd_gates_batch call over `jobs`; misalign = (job index, operand) / da_offset = job index whose da is misaligned.
    Returns [(da, dc_prev)] (Guarded)."""
    from rsis_amd import _lib
    from rsis_amd._lib import check, lib, ptr, stream
    arr = (_lib.LstmBwdJob * len(jobs))()
    keep, outs = [], []
    for k, (j, q) in enumerate(zip(arr, jobs)):
        d = _dev(q, misalign[1] if misalign is not None and misalign[0] == k else None)
        da, dcp = _outputs(q, offset=1 if da_offset == k else 0)
        B, hid, H, W = q["shape"]
        j.dh, j.dh2, j.dc_next, j.act, j.c_prev, j.c = [ptr(d[n]) for n in _IN]
        j.da, j.dc_prev = ptr(da.t), ptr(dcp.t) if dcp is not None else None
        j.B, j.hid, j.HW = B, hid, H * W
        keep.append(d)
        outs.append((da, dcp))
    check(lib().rsis_convlstm_bwd_gates_batch(arr, len(jobs), stream()), "rsis_convlstm_bwd_gates_batch")
    torch.cuda.synchronize()
    return outs


def _check_batch(what, jobs, outs):
    record = []
    for k, (q, (da, dcp)) in enumerate(zip(jobs, outs)):
        _check_job("%s job %d" % (what, k), q, da, dcp, record)
    print("\nBWD-OPS lstm_bwd %s: worst ratio %.2f (k = %d)" % (what, max(record), LSTM_BWD_K))


@pytest.mark.parametrize("c_scale", [1.0, 4.0], ids=["c1", "c4"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", LSTM_SHAPES, ids=_lstm_id)
def test_lstm_bwd_single_call(shape, form, c_scale):
    """rsis_convlstm_bwd_gates (lstm_bwd_kernel) with da_sum: the bars on da / dc_prev, and da_sum bit-equal to prefill + da in fp32"""
    q = _job(shape, form, 300 + shape[1], c_scale)
    d = _dev(q)
    da, dcp = _outputs(q)
    B, hid, H, W = shape
    pre = _t(_rng(310 + hid, (B, 4 * hid, H * W))).cuda()
    da_sum = Guarded((B, 4 * hid, H * W), init=pre)
    _single(q, d, da, dcp, da_sum.t)
    record = []
    _check_job("single call", q, da, dcp, record)
    print("\nBWD-OPS lstm_bwd single %s %s c scale %g: worst ratio %.2f" % (_lstm_id(shape), form, c_scale, record[0]))
    da_sum.check("da_sum")
    assert torch.equal(da_sum.t, pre + da.t), "da_sum != prefill + da (fp32)"


def _mixed_jobs(shapes, seed, c_scales=(1.0, 4.0)):
    forms = list(FORMS)
    return [_job(s, forms[k % 3], seed + k, c_scales[k % 2]) for k, s in enumerate(shapes)]


def test_lstm_bwd_batch_scalar_group():
    """all five shapes, the three forms mixed, one launch: (2, 3, 6, 5) has HW % 4 != 0, so the whole group runs lstm_bwd_group_kernel"""
    jobs = _mixed_jobs(LSTM_SHAPES, 400)
    _check_batch("scalar group (5 jobs)", jobs, _batch(jobs))
    jobs = _mixed_jobs(LSTM_SHAPES[::-1], 410, (4.0, 1.0))                 # every shape meets another form and scale
    _check_batch("scalar group (5 jobs, reversed)", jobs, _batch(jobs))


def test_lstm_bwd_batch_v4_group_and_single_call():
    """the three shapes with HW % 4 == 0 in one launch (lstm_bwd_group_v4_kernel), each job in every form across the three launches; the
    scalar single call of the same jobs is inside the same bars (no bit-equality: the two bodies may be contracted differently)"""
    for rot in range(3):
        forms = [list(FORMS)[(k + rot) % 3] for k in range(3)]
        jobs = [_job(s, f, 420 + 3 * rot + k, (1.0, 4.0)[(k + rot) % 2]) for k, (s, f) in enumerate(zip(V4_SHAPES, forms))]
        _check_batch("v4 group (forms %s)" % ",".join(forms), jobs, _batch(jobs))
        record = []
        for k, q in enumerate(jobs):
            da, dcp = _outputs(q)
            _single(q, _dev(q), da, dcp)
            _check_job("single call of v4 job %d" % k, q, da, dcp, record)


@pytest.mark.parametrize("which", ["dh", "act", "c", "dc_next", "da"])
def test_lstm_bwd_batch_misaligned_operand_falls_back(which):
    """the v4 shapes with one tensor of the middle job at a storage offset of 1 float: the launcher must run the scalar kernel (the v4
    kernel's 16-byte accesses on such a pointer would read and write the wrong floats)"""
    assert len(V4_SHAPES) == 3
    jobs = [_job(s, "full", 440 + k, (1.0, 4.0)[k % 2]) for k, s in enumerate(V4_SHAPES)]
    outs = _batch(jobs, misalign=(1, which) if which != "da" else None, da_offset=1 if which == "da" else None)
    _check_batch("misaligned %s" % which, jobs, outs)


def test_lstm_bwd_batch_nine_jobs_two_launches():
    """more than RSIS_LB_MAXJ = 8 jobs behind one call: eight v4 jobs, then (2, 3, 6, 5) alone in a second, scalar launch"""
    shapes = [V4_SHAPES[k % 3] for k in range(8)] + [LSTM_SHAPES[4]]
    jobs = _mixed_jobs(shapes, 460)
    assert jobs[8]["form"] == "last" and jobs[7]["form"] == "t0"
    _check_batch("nine jobs", jobs, _batch(jobs))


@pytest.mark.parametrize("kernel", ["v4", "scalar"])
def test_lstm_bwd_group_non_finite_cell_state(kernel):
    """c = +-inf and +-1e30 in a last-step job (dh2, dc_next absent) and a t = 0 job (c_prev absent): every output is finite and inside
    the bars of the float64 reference (tanh = +-1, 1 - tanh^2 = 0).  The v4 kernel loads absent operands from `c` and must SELECT them
    away -- a multiplication by 0 would give NaN here; the scalar kernel (forced by a job with HW % 4 != 0) never loads them."""
    jobs = [_job(V4_SHAPES[0], "last", 480, 4.0, nonfinite=True), _job(V4_SHAPES[1], "t0", 481, 1.0, nonfinite=True),
            _job(V4_SHAPES[2], "full", 482, 4.0, nonfinite=True)]
    if kernel == "scalar":
        jobs += [_job(LSTM_SHAPES[4], "last", 483, 1.0, nonfinite=True), _job(LSTM_SHAPES[0], "t0", 484, 4.0, nonfinite=True)]
    _check_batch("non-finite c, %s group" % kernel, jobs, _batch(jobs))


# ---------------------------------------------------------------- rsis_bias_grad
BIAS_CASES = [
    # (B, C, HW, lstm_hid)
    (2, 16, 35, 4),          # scalar path, permuted rows
    (3, 32, 64, 8),          # float4 path
    (2, 5, 12, 0),           # no permutation
    (4, 512, 16, 128),       # the widest gate layer
    (3, 4, 1000, 1),         # default mode takes 3 splits, float4 path
    (3, 4, 999, 1),          # default mode takes 3 splits, scalar path
]


def _bias_ref(dy, db0, hid):
    """float64: db[row(c)] = prefill[row(c)] + sum over (b, pixel) of dy[b][c], row(c) = (c % 4) hid + c // 4 on gate rows"""
    C = dy.shape[1]
    rows = np.array([(c % 4) * hid + c // 4 if hid > 0 else c for c in range(C)])
    assert sorted(rows.tolist()) == list(range(C))
    ref = db0.astype(np.float64).copy()
    ref[rows] += dy.astype(np.float64).sum((0, 2))
    mag = np.abs(db0).astype(np.float64)
    mag[rows] += np.abs(dy).astype(np.float64).sum((0, 2))
    return ref, mag


def _bias_run(dy, db0, hid):
    from rsis_amd._lib import check, lib, ptr, stream
    B, C, HW = dy.shape
    dyd = _t(dy).cuda()
    db = Guarded((C,), init=_t(db0))
    check(lib().rsis_bias_grad(ptr(dyd), ptr(db.t), B, C, HW, hid, stream()), "rsis_bias_grad")
    torch.cuda.synchronize()
    db.check("db")
    return db.t.double().cpu().numpy()


@pytest.mark.parametrize("case", BIAS_CASES, ids=lambda c: "B%d_C%d_HW%d_hid%d" % c)
def test_bias_grad_exact(case, mode):
    B, C, HW, hid = case
    dy, db0 = _ints(500 + C, (B, C, HW)), _ints(501 + C, (C,), -9, 9, nonzero=True)
    ref, mag = _bias_ref(dy, db0, hid)
    assert mag.max() < EXACT_LIMIT
    got = _bias_run(dy, db0, hid)
    bad = got != ref
    assert not bad.any(), "%s mode: %d of %d rows differ from the float64 reference in the exact regime (first %d: got %g want %g)" % (
        mode, bad.sum(), C, np.argmax(bad), got[np.argmax(bad)], ref[np.argmax(bad)])


@pytest.mark.parametrize("case", BIAS_CASES, ids=lambda c: "B%d_C%d_HW%d_hid%d" % c)
def test_bias_grad_normal(case, mode):
    """deterministic mode: the per-channel sum is formed in double by one block, so only the cast to fp32 and the add to the prefill round.
    Default mode (several blocks of a channel meet in fp32 atomics): the error is recorded, exactness covers the indexing."""
    B, C, HW, hid = case
    dy, db0 = _rng(510 + C, (B, C, HW)), _rng(511 + C, (C,))
    ref, _mag = _bias_ref(dy, db0, hid)
    got = _bias_run(dy, db0, hid)
    bar = 4 * 2.0 ** -24 * (np.abs(db0).astype(np.float64) + np.abs(ref))
    err = np.abs(got - ref)
    print("\nBWD-OPS bias_grad %r, %s mode: max err %.3e, worst err / bar %.3f" % (case, mode, err.max(), (err / bar).max()))
    if mode == "deterministic":
        assert (err <= bar).all(), "row %d: err %.3e > 4 * 2^-24 * (|prefill| + |ref|) = %.3e" % (np.argmax(err / bar), err[np.argmax(err / bar)],
                                                                                                 bar[np.argmax(err / bar)])


# ---------------------------------------------------------------- rsis_sum_leading
@pytest.mark.parametrize("T,n,offset", [(1, 7, 0), (10, 4096, 0), (3, 1027, 0), (20, 280, 0), (4, 1024, 1)],
                         ids=["T1_n7", "T10_n4096", "T3_n1027", "T20_n280", "T4_n1024_misaligned"])
def test_sum_leading_is_the_fixed_order_fp32_sum(T, n, offset):
    from rsis_amd._lib import check, lib, ptr, stream
    buf = torch.empty(T * n + offset, device="cuda")
    x = buf[offset:].view(T, n)
    x.copy_(_t(_rng(600 + T, (T, n))))
    assert x.data_ptr() % 16 == 4 * offset
    y = Guarded((n,))
    check(lib().rsis_sum_leading(ptr(x), ptr(y.t), T, n, stream()), "rsis_sum_leading")
    torch.cuda.synchronize()
    y.check("y")
    acc = x[0].clone()
    for t in range(1, T):
        acc = acc + x[t]
    assert torch.equal(y.t, acc), "y != x[0] + x[1] + ... in fp32, t ascending: %d of %d elements differ" % (int((y.t != acc).sum()), n)
    xi = _ints(610 + T, (T, n))                                        # exact regime: equal to the float64 sum
    x.copy_(_t(xi))
    y = Guarded((n,))
    check(lib().rsis_sum_leading(ptr(x), ptr(y.t), T, n, stream()), "rsis_sum_leading")
    torch.cuda.synchronize()
    y.check("y (exact regime)")
    assert np.array_equal(y.t.double().cpu().numpy(), xi.astype(np.float64).sum(0))
