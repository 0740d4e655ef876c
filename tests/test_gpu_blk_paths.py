"""The storage half of `-dtype bf16` against FLOAT64, bit for bit, op by op through the C ABI: rsis_blk_conv2d / rsis_blk_conv2d_bn_eval
(csrc/conv_blk.hip), the plain epilogue of rsis_blk_conv3x3_batch (csrc/conv_blk_dec.hip), rsis_blk_bn_fwd / rsis_blk_bn_bwd and the layout
helpers rsis_blk_from_nchw / _to_nchw / _subsample2d / _upscatter2d (csrc/blk_norm.hip).  Cases, builders, references, rounding helpers and host models: blk_paths_cases.py (checked by test_blk_paths_host.py).

The kernels promise fp32 arithmetic on exact bf16 inputs and ONE round-to-nearest-even at the blk store.  The 2^-8 relative bar of
test_gpu_blk.py accepts a truncating store, a double rounding and a tie broken the wrong way; here a stored value must BE the right one:

  * EXACT (indexing, rounding mode): integers in -3..3, sum |terms| < 2^24 (asserted on the host), so the fp32 accumulation is exact in
    any order, MFMA included, and the output must EQUAL bf16_rne64(float64 reference) -- on `index` cases every output is itself a bf16
    value (a lost or doubled tap of +-1 shows), on `round` cases 8-15 % of the outputs are not and as many are exact ties.  BatchNorm:
    integer x (-3..3, and 13..19 where E[x^2] - m^2 cancels) makes the statistics exact in double: save_mean within 1 ulp, save_rstd
    within 1 + (ceil(R) + 1) ulp (R: rsqrtf, probed below), the running statistics within 2 ulp, dbeta EQUAL on an integer prefill.
    A cell lost or doubled at a split boundary, or N - 1 for N, is thousands of ulps.
  * NORMAL (rounding): bf16-valued N(0.5, 2) and N(16, 2).  Every blk output goes through nearest_check: the bf16 nearest to the float64
    reference, or one of its two neighbours where the reference is within `delta` of their midpoint (delta: a rounding count times 2^-24
    times the magnitudes that enter, plus the sums' bars times the element's sensitivity; at most 1 % of a case is undecided, asserted
    on the host).  Sums (save_mean, save_rstd, dbeta, dgamma): err_gpu <= M_BN * err_host; err_host = the error of the numpy fp32 model that sums
    in the launch's own order (wave_sums: per-thread chains, the 64-lane fold, double above; bn_plan says why ONE sequential chain is
    no yardstick on N(16, 2) data) and carries the final fp32 conversions and rsqrtf as a unit within ceil(R) ulp of the root (the largest
    error over rstd - 1 ulp, rstd, rstd + 1 ulp).  M_BN is TWICE the worst err_gpu / err_host measured on
    the MI355X over all cases and both modes (NOTES.md (93), profiles/r19_a_blk_path_margins.txt) and must stay <= 4.

Every output is a guarded view (sentinels on each side, the view prefilled), checked after the call; every test runs in the default and
in the deterministic mode; forward and backward are run twice for equal bits.  One line per normal case and quantity is printed (with
RSIS_BLK_PATH_MARGINS=<file> the lines are appended there: the margin survey).

The ConvLSTM epilogue of rsis_blk_conv3x3_batch (section 6) runs on dyadic data, so every gate pre-activation is exact in fp32 and the
only errors are those of rsis_sigmoid_fast / rsis_tanh_fast and a few roundings.  Their worst absolute error E_F is PROBED on the device
through the cell state (fp32): with the g pre-activation at 32 the cell of a zero state is c = sigmoid_fast(a_i) * 1, with the i
pre-activation at 32 it is c = 1 * tanh_fast(a_g).  c is held to 2.25 E_F + 4 * 2^-24 max(1, |c|), h and act to nearest_check with
deltas from the same chain (blk_paths_cases.py).

Not covered here: RSIS_BLK_BN_BLOCK, RSIS_BLK_BN_MINCELLS and RSIS_BLKDEC_NR are read once per process and stay untested; a bias in the
ConvLSTM epilogue stays with test_gpu_blk_dec.py."""
import os

import numpy as np
import pytest
import torch

import blk_paths_cases as K
from helpers import Guarded

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(params=["default", "deterministic"])
def mode(request):
    from rsis_amd import ops
    prev = ops.set_deterministic(request.param == "deterministic")
    yield request.param
    ops.set_deterministic(prev)


def _abi():
    from rsis_amd import _lib
    return _lib


def _record(kind, cid, mode, what, err_host, err_gpu):
    ratio = err_gpu / err_host if err_host > 0 else (0.0 if err_gpu == 0 else float("inf"))
    line = "%-5s %-34s %-13s %-7s err_host %.3e  err_gpu %.3e  ratio %.3f" % (kind, cid, mode, what, err_host, err_gpu, ratio)
    print(line)
    if os.environ.get("RSIS_BLK_PATH_MARGINS"):
        with open(os.environ["RSIS_BLK_PATH_MARGINS"], "a") as f:
            f.write(line + "\n")
    return ratio


_DATA = {}


def _cached(key, build):
    """host inputs, float64 references and host models of a case, computed once and shared by the modes (never modified)"""
    if key not in _DATA:
        _DATA[key] = build()
    return _DATA[key]


def _blk(a):
    """bf16-valued float64 NCHW (numpy) -> blk tensor on the device"""
    t = torch.from_numpy(K.to_blk64(a)).to(torch.bfloat16)
    assert torch.equal(t.double(), torch.from_numpy(K.to_blk64(a))), "the input is not bf16-valued"
    return t.cuda()


def _nchw(t):
    """blk tensor -> float64 NCHW (numpy)"""
    return K.from_blk64(t.detach().double().cpu().numpy())


def _f32(a):
    return torch.from_numpy(np.asarray(a, np.float64)).float().cuda()


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.int16).cpu()


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(F32)).astype(np.float64)


# ======================================================================================================================
# 1. BatchNorm
# ======================================================================================================================
class _Scratch(object):
    """rsis_blk_bn_scratch_doubles(C) doubles and a sentinel tail"""

    def __init__(self, C):
        self.n = int(_abi().lib().rsis_blk_bn_scratch_doubles(int(C)))
        self.buf = torch.full((self.n + 64,), -7.5, dtype=torch.float64, device="cuda")

    def check(self):
        assert bool((self.buf[self.n:] == -7.5).all()), "the scratch buffer was overrun"


def bn_fwd(x, res, gamma, beta, rm, rv, relu, train, eps=K.BN_EPS):
    """rsis_blk_bn_fwd into guarded outputs: (y, save_mean, save_rstd, run_mean, run_var) as device tensors"""
    A = _abi()
    B, Cb, H, W, _ = x.shape
    C = Cb * 8
    y, sm, sr = K.GuardedBlk(tuple(x.shape)), Guarded((C,)), Guarded((C,))
    RM, RV = Guarded((C,), init=rm), Guarded((C,), init=rv)
    sc = _Scratch(C)
    A.check(A.lib().rsis_blk_bn_fwd(A.ptr(x), A.ptr(res), A.ptr(y.t), A.ptr(sc.buf), A.ptr(gamma), A.ptr(beta), A.ptr(RM.t), A.ptr(RV.t), A.ptr(sm.t),
                                    A.ptr(sr.t), B, C, H, W, float(eps), float(K.BN_MOMENTUM), int(relu), int(train), A.stream()), "rsis_blk_bn_fwd")
    torch.cuda.synchronize()
    for g, what in ((y, "y"), (sm, "save_mean"), (sr, "save_rstd"), (RM, "running_mean"), (RV, "running_var")):
        g.check(what)
    sc.check()
    if not train:
        assert sm.untouched() and sr.untouched(), "eval mode wrote the saved statistics"
    return y.t, sm.t, sr.t, RM.t, RV.t


def bn_bwd(dy, x, y, gamma, beta, sm, sr, relu, want_dres, dg0=None, db0=None, accumulate=False, null_params=False):
    """rsis_blk_bn_bwd into guarded outputs: (dx, dres or None, dgamma, dbeta)"""
    A = _abi()
    B, Cb, H, W, _ = x.shape
    C = Cb * 8
    dx = K.GuardedBlk(tuple(x.shape))
    dres = K.GuardedBlk(tuple(x.shape)) if want_dres else None
    dg, db = Guarded((C,), init=dg0), Guarded((C,), init=db0)
    sc = _Scratch(C)
    A.check(A.lib().rsis_blk_bn_bwd(A.ptr(dy), A.ptr(x), A.ptr(y), A.ptr(sc.buf), A.ptr(gamma), A.ptr(beta), A.ptr(sm), A.ptr(sr), A.ptr(dx.t),
                                    A.ptr(dres.t) if want_dres else None, None if null_params else A.ptr(dg.t), None if null_params else A.ptr(db.t),
                                    int(accumulate), B, C, H, W, int(relu), A.stream()), "rsis_blk_bn_bwd")
    torch.cuda.synchronize()
    for g, what in ((dx, "dx"), (dres, "dres"), (dg, "dgamma"), (db, "dbeta")):
        if g is not None:
            g.check(what)
    sc.check()
    if null_params:
        assert dg.untouched() and db.untouched()
    return dx.t, dres.t if want_dres else None, dg.t, db.t


def _bn_params(cases):
    return [pytest.param(c, id=K.bn_id(c)) for c in cases]


def _np(t):
    return t.detach().double().cpu().numpy()


def test_device_rsqrt_is_exact_at_powers_of_two(mode):
    """the precondition of the bn_eval expectations ON THE DEVICE, and the anchor of R: two cells +-s per channel give mean 0 and variance
    s^2 exactly; with eps = 0 save_rstd must be exactly 1 / s for s^2 in RSQRT_POW2"""
    s = np.array([0.25, 0.5, 1.0, 2.0, 4.0, 0.25, 1.0, 4.0])
    assert set((s * s).tolist()) == set(K.RSQRT_POW2)
    x = np.stack([s, -s]).reshape(2, 8, 1, 1)
    one, zero = _f32(np.ones(8)), _f32(np.zeros(8))
    _y, sm, sr, _rm, _rv = bn_fwd(_blk(x), None, one, zero, zero, one, False, True, eps=0.0)
    assert _np(sm).tolist() == [0.0] * 8 and _np(sr).tolist() == (1.0 / s).tolist()
    # eval mode takes rsqrtf(running_var + eps) in the apply kernel: y = x / s = +-1
    y, _sm, _sr, _rm, _rv = bn_fwd(_blk(x), None, one, zero, zero, _f32(s * s), False, False, eps=0.0)
    assert np.array_equal(_nchw(y), np.sign(x))


@pytest.mark.parametrize("regime", sorted(K.BN_EXACT_SETS))
@pytest.mark.parametrize("c", _bn_params(K.BN_CASES))
def test_bn_exact_statistics(c, regime, mode):
    """integer x: sum x and sum x^2 of every fp32 chain are exact, so the statistics are those of float64 up to the fp32 operations behind
    the sums -- and dbeta (integer dy, the mask of the product's own y) EQUALS float64 on top of an integer prefill"""
    d = _cached(("bn_in", K.bn_id(c), regime), lambda: K.bn_inputs(c, regime))
    st = _cached(("bn_st", K.bn_id(c), regime), lambda: K.bn_stats64(d["x"]))
    C, N = c["C"], st["N"]
    sign = np.where(st["mean"] < 0, -1.0, 1.0)
    rm0, rv0 = 0.5 * sign, np.full(C, 0.5)                 # same sign as the batch mean: the update does not cancel
    x = _blk(d["x"])
    gamma, beta = _f32(d["gamma"]), _f32(d["beta"])
    y, sm, sr, rm, rv = bn_fwd(x, None, gamma, beta, _f32(rm0), _f32(rv0), True, True)
    e_mean = np.abs(_np(sm) - st["mean"]) / _ulp32(st["mean"])
    e_rstd = np.abs(_np(sr) - st["rstd"]) / _ulp32(st["rstd"])
    # R of rsqrtf at this case's own arguments: against float64 on the fp32 argument the kernel forms
    arg = (st["var"].astype(F32) + F32(K.BN_EPS)).astype(np.float64)
    r_ulp = np.abs(_np(sr) - 1.0 / np.sqrt(arg)) / _ulp32(1.0 / np.sqrt(arg))
    _record("rsqrt", K.bn_id(c) + "/" + regime, mode, "R_ulp", 1.0, float(r_ulp.max()))
    assert e_mean.max() <= 1.0, "save_mean: %.2f ulp" % e_mean.max()
    assert e_rstd.max() <= K.K_RSTD_ULP, "save_rstd: %.2f ulp" % e_rstd.max()
    mom = K.BN_MOMENTUM
    want_rm, want_rv = (1 - mom) * rm0 + mom * st["mean"], (1 - mom) * rv0 + mom * st["unb"]
    assert (np.abs(_np(rm) - want_rm) <= 2 * _ulp32(want_rm)).all(), "running_mean: %.2f ulp" % (np.abs(_np(rm) - want_rm) / _ulp32(want_rm)).max()
    assert (np.abs(_np(rv) - want_rv) <= 2 * _ulp32(want_rv)).all(), "running_var: %.2f ulp" % (np.abs(_np(rv) - want_rv) / _ulp32(want_rv)).max()
    mask = _nchw(y) > 0
    assert 0.02 < mask.mean() < 0.98
    want_db = d["db0"] + (d["dy"] * mask).sum((0, 2, 3))
    for y_arg in (y, None):
        _dx, dres, _dg, db = bn_bwd(_blk(d["dy"]), x, y_arg, gamma, beta, sm, sr, True, True, dg0=_f32(d["dg0"]), db0=_f32(d["db0"]), accumulate=True)
        assert np.array_equal(_np(db), want_db), "dbeta (y %s)" % ("given" if y_arg is not None else "NULL")
        assert np.array_equal(_nchw(dres), d["dy"] * mask), "dres is dy under the mask of the stored y, exactly"


def _normal_refs(c, regime, relu, res):
    d = _cached(("bn_in", K.bn_id(c), regime), lambda: K.bn_inputs(c, regime))
    f = K.bn_fwd64(d, relu, res)
    m = K.bn_model32(d, c, relu, res)
    bm = K.bn_bwd64(d, f["st"], m["mask"])
    return d, f, m, K.bn_sum_errors(m, f, bm)


@pytest.mark.parametrize("regime", sorted(K.BN_NORMAL_SETS))
@pytest.mark.parametrize("relu,res", [(True, False), (True, True), (False, False)], ids=["relu", "relu_res", "plain"])
@pytest.mark.parametrize("c", _bn_params(K.BN_CASES))
def test_bn_normal(c, relu, res, regime, mode):
    """train-mode BatchNorm (+ residual) (+ ReLU), forward and backward, against float64 computed from float64 statistics (the residual
    added and the ReLU taken in float64).  y, dx: nearest_check (dx where the float64 pre-activation is clear of the ReLU's kink, by the
    rule of test_gpu_blk.py, more than 90 % of the elements); dres EQUALS dy under the mask of the stored y; sums: M_BN * err_host."""
    cid = "%s/%s/%s" % (K.bn_id(c), regime, "relu_res" if res else "relu" if relu else "plain")
    d, f, m, eh = _cached(("bn_n", cid), lambda: _normal_refs(c, regime, relu, res))
    st, N = f["st"], f["st"]["N"]
    x, gamma, beta = _blk(d["x"]), _f32(d["gamma"]), _f32(d["beta"])
    r = _blk(d["res"]) if res else None
    y, sm, sr, rm, rv = bn_fwd(x, r, gamma, beta, _f32(d["rm"]), _f32(d["rv"]), relu, True)
    y2, sm2, sr2, _rm2, _rv2 = bn_fwd(x, r, gamma, beta, _f32(d["rm"]), _f32(d["rv"]), relu, True)
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(sm, sm2) and torch.equal(sr, sr2), "two forward runs differ in bits"
    # ---- sums of the forward: err_gpu <= M_BN * err_host
    eg_mean = float(np.abs(_np(sm) - st["mean"]).max())
    eg_rstd = float((np.abs(_np(sr) - st["rstd"]) / st["rstd"]).max())
    _record("bn", cid, mode, "mean", eh["mean"], eg_mean)
    _record("bn", cid, mode, "rstd", eh["rstd"], eg_rstd)
    bar_mean, bar_rstd = K.M_BN * eh["mean"], K.M_BN * eh["rstd"]
    assert eg_mean <= bar_mean, "save_mean: err %.3e, M_BN x err_host %.3e" % (eg_mean, bar_mean)
    assert eg_rstd <= bar_rstd, "save_rstd (relative): err %.3e, M_BN x err_host %.3e" % (eg_rstd, bar_rstd)
    if N > 1:
        for got, want, what in ((rm, f["rm"], "running_mean"), (rv, f["rv"], "running_var")):
            # the update is three fp32 operations on top of the statistic's own error (the test of the exact regime pins it to 2 ulp)
            sens = K.BN_MOMENTUM * (bar_mean if what == "running_mean" else 2 * bar_rstd * st["unb"].max())
            assert (np.abs(_np(got) - want) <= 2 * _ulp32(want) + sens).all(), what
    # ---- y
    K.assert_nearest("y " + cid, _nchw(y), f["y"], K.bn_delta_y(d, f, res, bar_mean, bar_rstd))
    # ---- backward: the mask of the reference is that of the product's stored y
    mask = (_nchw(y) > 0) if relu else np.ones(d["x"].shape, bool)
    clear = K.clear_of_zero(f["pre"], relu)
    assert clear.mean() > 0.9
    if relu:
        assert np.array_equal(mask[clear], (f["pre"] > 0)[clear]), "the stored y has the wrong sign where the pre-activation is clear of zero"
    b = K.bn_bwd64(d, st, mask)
    dy = _blk(d["dy"])
    y_arg = y if res else None                     # (a residual needs the stored y; without one the mask is recomputed from x)
    dx, dres, dg, db = bn_bwd(dy, x, y_arg, gamma, beta, sm, sr, relu, True)
    dx2, dres2, dg2, db2 = bn_bwd(dy, x, y_arg, gamma, beta, sm, sr, relu, True)
    assert torch.equal(_bits(dx), _bits(dx2)) and torch.equal(_bits(dres), _bits(dres2)) and torch.equal(dg, dg2) and torch.equal(db, db2), \
        "two backward runs differ in bits"
    assert np.array_equal(_nchw(dres), b["g"]), "dres is dy under the mask of the stored y, exactly"
    eg_db, eg_dg = float(np.abs(_np(db) - b["dbeta"]).max()), float(np.abs(_np(dg) - b["dgamma"]).max())
    _record("bn", cid, mode, "dbeta", eh["dbeta"], eg_db)
    _record("bn", cid, mode, "dgamma", eh["dgamma"], eg_dg)
    bar_db, bar_dg = K.M_BN * eh["dbeta"], K.M_BN * eh["dgamma"]
    assert eg_db <= bar_db, "dbeta: err %.3e, M_BN x err_host %.3e" % (eg_db, bar_db)
    assert eg_dg <= bar_dg, "dgamma: err %.3e, M_BN x err_host %.3e" % (eg_dg, bar_dg)
    delta = K.bn_delta_dx(d, st, b, bar_mean, bar_rstd, bar_db, bar_dg)
    if N <= 2:
        # two cells per channel: dx is pure cancellation (the reference is ~0), its nearest bf16 says nothing: absolute, delta + half a bf16 step
        _lo, ulp = K.bf16_floor_ulp(np.abs(b["dx"]))
        assert (np.abs(_nchw(dx) - b["dx"]) <= delta + ulp / 2).all()
    else:
        K.assert_nearest("dx " + cid, _nchw(dx), b["dx"], delta, where=clear)


@pytest.mark.parametrize("regime", ["far", "n16"])
@pytest.mark.parametrize("c", _bn_params(K.BN_CASES))
def test_bn_backward_recomputed_mask_has_the_bits_of_the_stored_one(c, regime, mode):
    """relu without a residual: the backward with y_blk = NULL (mask recomputed as x * sc + sh > 0) has the BITS of the backward given the
    forward's y -- every kernel family (block kernels with and without y at NPT 4 / 8, the two-pass kernels), both regimes; and dgamma ==
    NULL / dbeta == NULL are accepted and leave dx unchanged"""
    d = _cached(("bn_in", K.bn_id(c), regime), lambda: K.bn_inputs(c, regime))
    x, dy, gamma, beta = _blk(d["x"]), _blk(d["dy"]), _f32(d["gamma"]), _f32(d["beta"])
    y, sm, sr, _rm, _rv = bn_fwd(x, None, gamma, beta, _f32(d["rm"]), _f32(d["rv"]), True, True)
    a = bn_bwd(dy, x, y, gamma, beta, sm, sr, True, True)
    b = bn_bwd(dy, x, None, gamma, beta, sm, sr, True, True)
    for p, q, what in zip(a, b, ("dx", "dres", "dgamma", "dbeta")):
        assert torch.equal(_bits(p) if p.dtype == torch.bfloat16 else p, _bits(q) if q.dtype == torch.bfloat16 else q), what
    n = bn_bwd(dy, x, None, gamma, beta, sm, sr, True, False, null_params=True)
    assert torch.equal(_bits(n[0]), _bits(a[0]))


@pytest.mark.parametrize("c", _bn_params(K.BN_EVAL_SHAPES))
def test_bn_eval_mode_uses_the_running_statistics(c, mode):
    """eval mode at the block / two-pass boundary shapes (always the apply kernel): y from the running statistics by nearest_check,
    save_* and the running statistics not written (guarded, prefilled)"""
    d = _cached(("bn_in", K.bn_id(c), "n05"), lambda: K.bn_inputs(c, "n05"))
    st = dict(N=c["B"] * c["H"] * c["W"], mean=d["rm"], var=d["rv"], rstd=1.0 / np.sqrt(d["rv"] + K.BN_EPS), unb=d["rv"])
    for relu, res in ((True, True), (False, False)):
        f = K.bn_fwd64(d, relu, res, st=st)
        y, _sm, _sr, rm, rv = bn_fwd(_blk(d["x"]), _blk(d["res"]) if res else None, _f32(d["gamma"]), _f32(d["beta"]), _f32(d["rm"]), _f32(d["rv"]), relu, False)
        assert np.array_equal(_np(rm), d["rm"]) and np.array_equal(_np(rv), d["rv"]), "eval mode changed the running statistics"
        K.assert_nearest("eval y", _nchw(y), f["y"], K.bn_delta_y(d, f, res, 0.0, 0.0))


def test_bn_store_rounds_ties_to_even(mode):
    """exact regime of the BatchNorm store (eval mode with sc = 1, sh = 1/2 on integers 128..255; rsqrtf(1) = 1 probed above): every unrounded
    output is a tie, and the stored value must be the EVEN neighbour -- a store that rounds half away from zero or truncates fails here"""
    d = K.bn_tie_data()
    y, _sm, _sr, _rm, _rv = bn_fwd(_blk(d["x"]), None, _f32(d["gamma"]), _f32(d["beta"]), _f32(d["rm"]), _f32(d["rv"]), False, False, eps=0.0)
    assert np.array_equal(_nchw(y), K.bf16_rne64(d["y"]))


# ======================================================================================================================
# 2. layout helpers
# ======================================================================================================================
def test_from_nchw_rounds_to_nearest_even(mode):
    """rsis_blk_from_nchw on ties, both fp32 neighbours of a tie, +-0, +-inf, NaN (stays NaN), fp32 denormals and the largest finite fp32"""
    A = _abi()
    v = K.from_nchw_specials()
    W = -(-v.size // 8)
    a = np.ones(W * 8)
    a[:v.size] = v
    x = torch.from_numpy(a.reshape(1, 8, 1, W)).float().cuda().contiguous()
    y = K.GuardedBlk((1, 1, 1, W, 8))
    A.check(A.lib().rsis_blk_from_nchw(A.ptr(x), A.ptr(y.t), 1, 8, 1, W, A.stream()), "rsis_blk_from_nchw")
    torch.cuda.synchronize()
    y.check("y")
    got, want = _nchw(y.t).reshape(-1), K.bf16_rne64(a)
    nan = np.isnan(a)
    assert np.isnan(got[nan]).all() and nan.sum() == 1
    bad = (got[~nan] != want[~nan]) | (np.signbit(got[~nan]) != np.signbit(want[~nan]))
    assert not bad.any(), "fp32 -> bf16: %s became %s, nearest-even is %s" % (a[~nan][bad][:6], got[~nan][bad][:6], want[~nan][bad][:6])


@pytest.mark.parametrize("hw", K.COPY_MAPS, ids=lambda s: "%dx%d" % s)
def test_exact_copies(hw, mode):
    """rsis_blk_to_nchw, rsis_blk_subsample2d and rsis_blk_upscatter2d reproduce their inputs exactly, into guarded outputs, at strides 2 and 3"""
    A = _abi()
    H, W = hw
    B, C = K.COPY_B, K.COPY_C
    rng = np.random.default_rng(H * 100 + W)
    x64 = K.bf16_rne64(rng.standard_normal((B, C, H, W)) * np.exp2(rng.integers(-20, 20, (B, C, H, W))))
    x = _blk(x64)
    out = Guarded((B, C, H, W))
    A.check(A.lib().rsis_blk_to_nchw(A.ptr(x), A.ptr(out.t), B, C, H, W, A.stream()), "rsis_blk_to_nchw")
    torch.cuda.synchronize()
    out.check("to_nchw")
    assert np.array_equal(_np(out.t), x64)
    for s in K.COPY_STRIDES:
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        sub = K.GuardedBlk((B, C // 8, Ho, Wo, 8))
        A.check(A.lib().rsis_blk_subsample2d(A.ptr(x), A.ptr(sub.t), B, C, H, W, s, A.stream()), "rsis_blk_subsample2d")
        torch.cuda.synchronize()
        sub.check("subsample")
        assert np.array_equal(_nchw(sub.t), x64[:, :, ::s, ::s])
        up = K.GuardedBlk((B, C // 8, H, W, 8))
        A.check(A.lib().rsis_blk_upscatter2d(A.ptr(sub.t), A.ptr(up.t), B, C, H, W, s, A.stream()), "rsis_blk_upscatter2d")
        torch.cuda.synchronize()
        up.check("upscatter")
        want = np.zeros_like(x64)
        want[:, :, ::s, ::s] = x64[:, :, ::s, ::s]
        assert np.array_equal(_nchw(up.t), want)


# ======================================================================================================================
# 3. rsis_blk_conv2d / rsis_blk_conv2d_bn_eval, exact regime
# ======================================================================================================================
def _conv_setup(c):
    """device inputs and the two bf16 packs of a case (built once; read-only)"""
    from rsis_amd import ops
    d = K.conv_exact_data(c)
    pk = ops.PackedConv(c["ks"], [c["Cin"]], stride=1, pad=c["ks"] // 2, dtype=ops.DTYPE_BF16)
    w = _f32(d["w"])
    return dict(d=d, x=_blk(d["x"]), dy=_blk(d["dy"]), add=_blk(d["add"]), wf=pk.fwd(w), wd=pk.dgrad(w), keep=(pk, w),
                want_y=K.bf16_rne64(d["y"]), want_dx=K.bf16_rne64(d["dx"]), want_dx0=K.bf16_rne64(d["dx"] - d["add"]))


def conv2d(x, wp, Cout, ks, variant, addend=None, alias=False, bn=None, relu=False, single_rounding=False):
    """rsis_blk_conv2d (or _bn_eval) into a guarded, prefilled output; alias: the addend is copied into the output and passed as that"""
    A = _abi()
    B, Cb, H, W, _ = x.shape
    out = K.GuardedBlk((B, Cout // 8, H, W, 8))
    if alias:
        out.t.copy_(addend)
        addend = out.t
    if bn is None:
        A.check(A.lib().rsis_blk_conv2d(A.ptr(x), B, Cb * 8, H, W, A.ptr(wp), Cout, ks, A.ptr(addend), A.ptr(out.t), int(variant), A.stream()), "rsis_blk_conv2d")
    else:
        g, b, m, v = bn
        A.check(A.lib().rsis_blk_conv2d_bn_eval(A.ptr(x), B, Cb * 8, H, W, A.ptr(wp), Cout, ks, A.ptr(addend), A.ptr(g), A.ptr(b), A.ptr(m), A.ptr(v), 0.0,
                                                int(relu), int(single_rounding), A.ptr(out.t), int(variant), A.stream()), "rsis_blk_conv2d_bn_eval")
    torch.cuda.synchronize()
    out.check("out")
    return out.t


def _conv_params(cases):
    return [pytest.param(c, v, id="%s-v%d" % (K.conv_id(c), v)) for c in cases for v in K.CONV_VARIANTS[c["ks"]]]


@pytest.mark.parametrize("c,variant", _conv_params(K.CONV_CASES))
def test_blk_conv2d_exact(c, variant, mode):
    """forward pack and data-gradient pack, every forced variant and variant 0 (its dispatch branches are covered by the maps of the case
    table): the output EQUALS bf16_rne64(float64) -- a NULL addend into a prefilled output, an addend, and (variant 0) an addend that
    aliases the output; forward and data gradient twice for equal bits"""
    s = _cached(("conv", K.conv_id(c)), lambda: _conv_setup(c))
    ks, Cin, Cout = c["ks"], c["Cin"], c["Cout"]
    y = conv2d(s["x"], s["wf"], Cout, ks, variant)
    assert np.array_equal(_nchw(y), s["want_y"]), "forward: %d of %d differ" % ((_nchw(y) != s["want_y"]).sum(), s["want_y"].size)
    assert torch.equal(_bits(y), _bits(conv2d(s["x"], s["wf"], Cout, ks, variant))), "two runs differ in bits"
    dx = conv2d(s["dy"], s["wd"], Cin, ks, variant, addend=s["add"])
    assert np.array_equal(_nchw(dx), s["want_dx"]), "data gradient + addend: %d of %d differ" % ((_nchw(dx) != s["want_dx"]).sum(), s["want_dx"].size)
    assert torch.equal(_bits(dx), _bits(conv2d(s["dy"], s["wd"], Cin, ks, variant, addend=s["add"]))), "two runs of the data gradient differ in bits"
    if variant == 0:
        dxa = conv2d(s["dy"], s["wd"], Cin, ks, 0, addend=s["add"], alias=True)
        assert torch.equal(_bits(dxa), _bits(dx)), "an addend that aliases the output"
        dx0 = conv2d(s["dy"], s["wd"], Cin, ks, 0)
        assert np.array_equal(_nchw(dx0), s["want_dx0"]), "data gradient without addend"


@pytest.mark.parametrize("c,variant", _conv_params(K.BN_EVAL_CASES))
def test_blk_conv2d_bn_eval_exact(c, variant, mode):
    """the eval-mode BatchNorm in the conv's epilogue with gamma, rsqrt(var) and the shift exact powers of two (eps = 0; rsqrtf probed above):
    single_rounding = 0 EQUALS the affine map of the bf16-rounded product, rounded again; single_rounding = 1 that of the exact product,
    rounded once -- the two differ on more than 1 % of the elements (asserted on the host)"""
    s = _cached(("conv", K.conv_id(c)), lambda: _conv_setup(c))
    p = _cached(("bn_eval", K.conv_id(c)), lambda: K.bn_eval_params(c))
    bn = tuple(_f32(p[k]) for k in ("gamma", "beta", "mean", "var"))
    for relu, res in ((False, False), (True, True)):
        r64 = p["res"] if res else None
        for single in (0, 1):
            got = conv2d(s["x"], s["wf"], c["Cout"], c["ks"], variant, addend=_blk(p["res"]) if res else None, bn=bn, relu=relu, single_rounding=single)
            want = K.bn_eval_expect(s["d"]["y"], p, r64, relu, single)
            assert np.array_equal(_nchw(got), want), "single_rounding %d, relu %d, res %d: %d of %d differ" % (single, relu, res, (_nchw(got) != want).sum(), want.size)


# ======================================================================================================================
# 4. rsis_blk_conv3x3_batch, plain epilogue, exact regime
# ======================================================================================================================
def _batch_setup(c):
    from rsis_amd import ops
    d = K.batch_exact_data(c)
    pk = ops.PackedConv(3, c["segs"], stride=1, pad=1, dtype=ops.DTYPE_BF16)
    w = _f32(d["w"])
    cuts = np.cumsum([0] + c["segs"])
    return dict(d=d, xs=[_blk(d["x"][:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], dy=_blk(d["dy"]), add=_blk(d["add_out"]), bias=_f32(d["bias"]),
                wf=pk.fwd(w), wd=pk.dgrad(w), cpack=pk.cin, keep=(pk, w),
                want_y=K.bf16_rne64(d["y"]), want_yb=K.bf16_rne64(d["yb"]), want_dx=K.bf16_rne64(d["dx0"]),
                want_bias=K.bf16_rne64(d["y"] + d["bias"][None, :, None, None]), want_add=K.bf16_rne64(d["y"] + d["add_out"]))


def _dsts(c_list, B, H, W):
    return [K.GuardedBlk((B, n // 8, H, W, 8)) for n in c_list]


def _cat(gs):
    return np.concatenate([_nchw(g.t) for g in gs], 1)


def _plain_jobs(c, s, tile):
    """the uses of a case as (job, guarded destinations, expected values): one destination; bias + addend over two destinations; bias alone;
    addend alone; the
    data gradient over the sources' channels (two destinations); the data gradient of the leading source only (Cout < Cpack)"""
    from rsis_amd import ops
    B, H, W, Cout, segs = c["B"], c["H"], c["W"], c["Cout"], c["segs"]
    out = []
    g = _dsts([Cout], B, H, W)
    out.append((ops.blk_conv_job(s["xs"], s["wf"], Cout, dsts=[x.t for x in g], tile=tile), g, s["want_y"]))
    g = _dsts(list(c["split"]) if c["split"] else [Cout], B, H, W)
    out.append((ops.blk_conv_job(s["xs"], s["wf"], Cout, bias=s["bias"], addend=s["add"], dsts=[x.t for x in g], tile=tile), g, s["want_yb"]))
    g = _dsts([Cout], B, H, W)                                             # bias alone, addend alone
    out.append((ops.blk_conv_job(s["xs"], s["wf"], Cout, bias=s["bias"], dsts=[x.t for x in g], tile=tile), g, s["want_bias"]))
    g = _dsts(list(c["split"]) if c["split"] else [Cout], B, H, W)
    out.append((ops.blk_conv_job(s["xs"], s["wf"], Cout, addend=s["add"], dsts=[x.t for x in g], tile=tile), g, s["want_add"]))
    cin = sum(segs)
    g = _dsts([segs[0], cin - segs[0]] if len(segs) > 1 else [cin], B, H, W)
    out.append((ops.blk_conv_job([s["dy"]], s["wd"], cin, cpack=s["cpack"], dsts=[x.t for x in g], tile=tile), g, s["want_dx"]))
    if len(segs) > 1:
        g = _dsts([segs[0]], B, H, W)
        out.append((ops.blk_conv_job([s["dy"]], s["wd"], segs[0], cpack=s["cpack"], dsts=[x.t for x in g], tile=tile), g, s["want_dx"][:, :segs[0]]))
    return out


@pytest.mark.parametrize("tile", K.BATCH_TILES)
@pytest.mark.parametrize("c", [pytest.param(c, id=K.batch_id(c)) for c in K.BATCH_CASES])
def test_blk_conv3x3_batch_plain_exact(c, tile, mode):
    """one, two and three sources with their channel tails, bias + addend, two destinations (one split inside a 32-row block), the data
    gradient and its leading destination alone, on both bd_body tiles: every output EQUALS bf16_rne64(float64)"""
    from rsis_amd import ops
    s = _cached(("batch", K.batch_id(c)), lambda: _batch_setup(c))
    for i, (job, g, want) in enumerate(_plain_jobs(c, s, tile)):
        ops.blk_conv3x3_batch([job])
        torch.cuda.synchronize()
        for x in g:
            x.check("use %d" % i)
        got = _cat(g)
        assert np.array_equal(got, want), "use %d: %d of %d differ" % (i, (got != want).sum(), want.size)


def test_blk_conv3x3_batch_grouped_launch_exact(mode):
    """ONE grouped launch of unlike jobs (every use of every case: different maps, sources, epilogues and tiles): each job EQUALS the
    reference, hence its single launch above"""
    from rsis_amd import ops
    jobs = []
    for k, c in enumerate(K.BATCH_CASES):
        s = _cached(("batch", K.batch_id(c)), lambda: _batch_setup(c))
        jobs += _plain_jobs(c, s, (0, 4, 5, 0)[k])
    assert len(jobs) >= 3
    ops.blk_conv3x3_batch([j for j, _g, _w in jobs])
    torch.cuda.synchronize()
    for i, (_j, g, want) in enumerate(jobs):
        for x in g:
            x.check("job %d" % i)
        assert np.array_equal(_cat(g), want), "job %d of the grouped launch" % i


# ======================================================================================================================
# 5. side keys of the ConvLSTM epilogue
# ======================================================================================================================
class _GuardedKeys(object):
    """the int64 key buffer [B][hid] (zero: the identity of the kernel's atomic max) between 64 sentinel elements on each side"""

    def __init__(self, B, hid):
        self.n = B * hid
        self.buf = torch.full((self.n + 128,), -7, dtype=torch.int64, device="cuda")
        self.buf[64:64 + self.n] = 0
        self.t = self.buf[64:64 + self.n].view(B, hid)

    def check(self):
        assert bool((self.buf[:64] == -7).all()) and bool((self.buf[64 + self.n:] == -7).all()), "side keys: a guard zone was written"


@pytest.mark.parametrize("tie", [True, False], ids=["tie", "spread"])
@pytest.mark.parametrize("c", [pytest.param(c, id=K.side_id(c)) for c in K.SIDE_CASES])
def test_side_keys_name_the_maximum_and_the_smallest_pixel(c, tie, mode):
    """the global max-pool keys of h on dyadic data (every pre-activation exact in fp32), with RSIS_SIDE_CHECK_TILES tiles per image (the
    path that reads the key before its atomic), just below, and on a small map without a source:
      * c within 2.25 E_F + 4 * 2^-24 max(1, |c|), h and act by nearest_check, as in section 6;
      * the decoded value is the float64 maximum of h over the image within the bar of h;
      * the stored h at the decoded pixel is the rounded decoded value, and it is the maximum of the stored map;
      * tie (zero weights, an addend constant over the pixels: every pixel of a channel holds the same h): the key names PIXEL 0."""
    d = _cached(("side", K.side_id(c), tie), lambda: K.side_data(c, tie))
    B, hid, cs, H, W = c["B"], c["hid"], c["csrc"], c["H"], c["W"]
    cg, h, act, key = lstm_cell(d["G"], hid, [_blk(d["x"])] if cs else [], d["w"], [max(cs, 8)], None, c["tile"], (B, H, W))
    err = np.abs(cg - d["c"])
    assert (err <= K.lstm_delta_c(d["c"])).all(), "c: %.3e over its bar at worst" % (err - K.lstm_delta_c(d["c"])).max()
    dh = K.lstm_delta_h(d["c"])
    K.assert_nearest("h", h, d["h"], dh)
    K.assert_nearest("act", act, d["act"], K.E_F)
    val, idx = K.key_decode(key)
    hs, h64 = h.reshape(B, hid, -1), d["h"].reshape(B, hid, -1)
    assert (idx >= 0).all() and (idx < H * W).all()
    at = np.take_along_axis(hs, idx[:, :, None], 2)[:, :, 0]
    assert np.array_equal(at, K.bf16_rne64(val)), "stored h at the pooled pixel != rounded pooled value"
    assert np.array_equal(at, hs.max(2)), "the pooled pixel does not hold the maximum of the stored map"
    gap = np.abs(val - h64.max(2))
    assert gap.max() <= float(np.max(dh)), "pooled value: %.3e from the float64 maximum, bar %.3e" % (gap.max(), float(np.max(dh)))
    if tie:
        assert (hs == hs[:, :, :1]).all(), "equal inputs, different h"
        assert (idx == 0).all(), "equal maxima: the key must name the smallest pixel index, got %s" % sorted(set(idx.reshape(-1).tolist()))[:8]


# ======================================================================================================================
# 6. ConvLSTM epilogue: the probe of the fast sigmoid / tanh, and c, h, act on dyadic data
# ======================================================================================================================
def lstm_cell(G, hid, srcs, w, segs, c_prev, tile, shape, keys=True):
    """one fused cell through rsis_blk_conv3x3_batch into guarded outputs: (c, h, act, key) ; G in reference row order [i | f | o | g] x hid"""
    from rsis_amd import ops
    B, H, W = shape
    pk = ops.PackedConv(3, segs, lstm_hid=hid, stride=1, pad=1, dtype=ops.DTYPE_BF16)
    wt = _f32(w)
    perm = np.arange(4 * hid).reshape(4, hid).T.reshape(-1)               # packed row 4 j + gate <- reference row gate * hid + j
    h, act = K.GuardedBlk((B, hid // 8, H, W, 8)), K.GuardedBlk((B, 4 * hid // 8, H, W, 8))
    cst, key = Guarded((B, hid, H, W)), _GuardedKeys(B, hid)
    job = ops.blk_conv_job(srcs, pk.fwd(wt), 4 * hid, addend=_blk(G[:, perm]), hid=hid, c_prev=c_prev, c_out=cst.t, h_out=h.t, act_out=act.t,
                           side_key=key.t if keys else None, tile=tile, shape=(B, H, W))
    ops.blk_conv3x3_batch([job])
    torch.cuda.synchronize()
    for g, what in ((h, "h"), (act, "act"), (cst, "c")):
        g.check(what)
    key.check()
    inv = np.argsort(perm)
    return _np(cst.t), _nchw(h.t), _nchw(act.t)[:, inv], key.t.cpu().numpy()


def test_fast_sigmoid_and_tanh_probe(mode):
    """E_F on the device: rsis_sigmoid_fast and rsis_tanh_fast, isolated in the fp32 cell state of a zero-state cell without sources (see the
    header), over the grid of the cases' pre-activations, against float64.  Beside it, for the record: the same expression with
    torch.exp2 / torch.reciprocal in fp32 on the device, and the float64 function of the fp32-ROUNDED scaled argument (argument
    rounding alone).  The worst device error must stay within E_F, the figure every ConvLSTM bar here is derived from."""
    v = K.fast_probe_args()
    hid, H = 8, 8
    W = -(-v.size // H)
    grid = np.zeros(H * W)
    grid[:v.size] = v
    grid = grid.reshape(1, 1, H, W)
    big = np.full((1, hid, H, W), 32.0)
    zero = np.zeros((1, hid, H, W))
    w = np.zeros((4 * hid, 8, 3, 3))
    x = torch.from_numpy(grid.reshape(-1)).float().cuda()
    worst = 0.0
    for name, G, f64, scale in (("sigmoid", np.concatenate([zero + grid, zero, zero, big], 1), lambda a: 1.0 / (1.0 + np.exp(-a)), K.LOG2E),
                                ("tanh", np.concatenate([big, zero, zero, zero + grid], 1), np.tanh, 2.0 * K.LOG2E)):
        c, _h, _act, _key = lstm_cell(G, hid, [], w, [8], None, 4, (1, H, W), keys=False)
        assert (c == c[:, :1]).all(), "every channel holds the same arguments"
        got = c[0, 0].reshape(-1)
        ref = f64(grid.reshape(-1))
        e_dev = float(np.abs(got - ref).max())
        t = torch.tensor(-scale, dtype=torch.float32, device="cuda") * x
        r = torch.reciprocal(1.0 + torch.exp2(t))
        rep = (r if name == "sigmoid" else 2.0 * r - 1.0).double().cpu().numpy()
        t64 = t.double().cpu().numpy()
        arg = 1.0 / (1.0 + np.exp2(t64))
        arg = arg if name == "sigmoid" else 2.0 * arg - 1.0
        _record("fast", name, mode, "E_dev", K.E_F, e_dev)
        _record("fast", name, mode, "E_torch", K.E_F, float(np.abs(rep - ref).max()))
        _record("fast", name, mode, "E_arg", K.E_F, float(np.abs(arg - ref).max()))
        worst = max(worst, e_dev)
    assert worst <= K.E_F, "the fast sigmoid / tanh are %.3e from float64 on the device: E_F = %.3e no longer holds" % (worst, K.E_F)


@pytest.mark.parametrize("state", [False, True], ids=["zero", "recurrent"])
@pytest.mark.parametrize("tile", K.LSTM_TILES)
@pytest.mark.parametrize("c", [pytest.param(c, id=K.lstm_id(c)) for c in K.LSTM_CASES])
def test_convlstm_epilogue_on_dyadic_data(c, tile, state, mode):
    """zero and recurrent state, nsrc = 0 (hid 16, zero state), tiles 4 and 5, hid 8 / 16 / 24: c within 2.25 E_F + 4 * 2^-24 max(1, |c|),
    h and act by nearest_check; the side key's value within the bar of h of the float64 maximum, the stored h at its pixel the rounded value"""
    d = _cached(("lstm", K.lstm_id(c), state), lambda: K.lstm_data(c, state))
    B, hid, cu, H, W = c["B"], c["hid"], c["c_up"], c["H"], c["W"]
    srcs = ([_blk(d["up"])] if cu else []) + ([_blk(d["h_prev"])] if state else [])
    segs = ([cu] if cu else []) + [hid]
    cg, h, act, key = lstm_cell(d["G"], hid, srcs, d["w"], segs, _f32(d["c_prev"]) if state else None, tile, (B, H, W))
    err = np.abs(cg - d["c"])
    assert (err <= K.lstm_delta_c(d["c"])).all(), "c: %.3e over its bar at worst" % (err - K.lstm_delta_c(d["c"])).max()
    dh = K.lstm_delta_h(d["c"])
    K.assert_nearest("h", h, d["h"], dh)
    K.assert_nearest("act", act, d["act"], K.E_F)
    val, idx = K.key_decode(key)
    hs, h64 = h.reshape(B, hid, -1), d["h"].reshape(B, hid, -1)
    at = np.take_along_axis(hs, idx[:, :, None], 2)[:, :, 0]
    assert np.array_equal(at, K.bf16_rne64(val)), "stored h at the pooled pixel != rounded pooled value"
    assert np.abs(val - h64.max(2)).max() <= float(np.max(dh)), "pooled value against the float64 maximum"
