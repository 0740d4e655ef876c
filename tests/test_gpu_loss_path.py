"""The loss path of the training step against FLOAT64 on the host, op by op through the C ABI: rsis_softiou_sums / rsis_softiou_bwd,
rsis_heads_fwd / rsis_heads_fwd_keys / rsis_heads_bwd, rsis_loss_tail (csrc/losses.hip) and rsis_assign_min_cost (the two assignment
kernels of csrc/pointwise.hip).  Cases, builders, references and host models: loss_path_cases.py (checked by test_loss_path_host.py).

Two data regimes, as in test_gpu_train_paths.py:

  * EXACT (coverage, indexing, masking): inputs for which every fp32 operation of the kernel is exact in any order, under any split and
    any atomics, so the result must EQUAL the float64 reference, in the default and in the deterministic mode.
      soft-IoU   logits from {-100, 0, +30} (fp32 sigmoid exactly 0, 1/2, 1: probed on the device below), masks in {0, 1}: every sum is a
                 count in halves below 2^23; p (1 - p) is 1/4 or 0 and ca / cb are small integers, so dlogits is exact too;
      heads      integers in -3..3 and probs 1 / 2^k: the stop logit, every d-logit and every gradient (on top of an integer prefill);
      assignment scores in multiples of 2^-20 below 16: the float64 total of any assignment is exact, so "optimal" is an EQUALITY with
                 scipy's optimum, ties included.
  * NORMAL (rounding): seeded Gaussian data in two spreads (`hot`: saturated sigmoids / softmax).  Bars against float64:
      sums       err_gpu <= M * err_host, both the largest error over the case, err_host that of the numpy model (fp32 operations, every
                 sum one sequential chain).  M_IOU and M_HEADS are TWICE the worst err_gpu / err_host measured on the MI355X over all
                 cases and both modes (NOTES.md (88), profiles/r14_a_loss_path_margins.txt) and must stay <= 4; M_TAIL is that cap
                 itself (test_loss_tail says why);
      soft-IoU cost = 1 - I / U, U = P + Y - I + e, from sums each within E = M_IOU * err_host: |dU| <= 3 E, so
                 |d(I / U)| <= E / U + I * 3 E / U^2 <= 4 E / U (I <= U); the fp32 evaluation adds three roundings of sums below 2 U
                 (6 u relative in U), the division and the subtraction (1 u each, on values <= 1): bar 4 E / U + 8 * 2^-24 per pair;
      elementwise outputs (dlogits, dsiou, dprobs, dstop): a rounding count * 2^-24, derived in loss_path_cases.py (K_*).

Every output is a guarded view (sentinels on each side), checked after the call.  One line per normal case is printed: err_host,
err_gpu, ratio (with RSIS_LOSS_PATH_MARGINS=<file> the lines are appended there: the margin survey)."""
import os
import types

import numpy as np
import pytest
import torch

import loss_path_cases as L
from helpers import Guarded, assert_close, to_tensor as _t

pytestmark = pytest.mark.gpu

OK, ERR_ARG, UNSUPPORTED = 0, 1, 3
U24 = L.U24


@pytest.fixture(params=["default", "deterministic"])
def mode(request):
    from rsis_amd import ops
    prev = ops.set_deterministic(request.param == "deterministic")
    yield request.param
    ops.set_deterministic(prev)


def _dev(a):
    return _t(a).cuda() if a is not None else None


def _abi():
    from rsis_amd import _lib
    return _lib


def _record(kind, cid, mode, err_host, err_gpu):
    ratio = err_gpu / err_host if err_host > 0 else (0.0 if err_gpu == 0 else float("inf"))
    line = "%-6s %-40s %-13s err_host %.3e  err_gpu %.3e  ratio %.3f" % (kind, cid, mode, err_host, err_gpu, ratio)
    print(line)
    if os.environ.get("RSIS_LOSS_PATH_MARGINS"):
        with open(os.environ["RSIS_LOSS_PATH_MARGINS"], "a") as f:
            f.write(line + "\n")
    return ratio


def _max_err(t, ref):
    return float(np.abs(t.detach().double().cpu().numpy() - ref).max())


class GuardedInt(object):
    """helpers.Guarded for an integer output (perm, arg-max pixels): 64 sentinel elements on each side of the view"""
    FILL = -7

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 128,), self.FILL, dtype=dtype, device="cuda")
        self.t = self.buf[64:64 + n].view(*shape)

    def check(self, what):
        assert bool((self.buf[:64] == self.FILL).all()) and bool((self.buf[-64:] == self.FILL).all()), "%s: a guard zone was written" % what


_DATA = {}


def _cached(key, build):
    """host inputs and float64 references of a case, computed once and shared by the modes (never modified)"""
    if key not in _DATA:
        _DATA[key] = build()
    return _DATA[key]


# ======================================================================================================================
# 1. soft-IoU
# ======================================================================================================================
def run_sums(logits, y):
    A = _abi()
    B, T, N = logits.shape
    G = y.shape[1]
    S = Guarded((B, T + 1, G + 1))
    A.check(A.lib().rsis_softiou_sums(A.ptr(logits), A.ptr(y), A.ptr(S.t), B, T, G, N, A.stream()), "rsis_softiou_sums")
    torch.cuda.synchronize()
    S.check("S")
    return S.t


def run_bwd(logits, y, perm, ca, cb):
    A = _abi()
    B, T, N = logits.shape
    d = Guarded((B, T, N))
    A.check(A.lib().rsis_softiou_bwd(A.ptr(logits), A.ptr(y), A.ptr(perm), perm.shape[1], A.ptr(ca), A.ptr(cb), A.ptr(d.t), B, T, y.shape[1], N,
                                     A.stream()), "rsis_softiou_bwd")
    torch.cuda.synchronize()
    d.check("dlogits")
    return d.t


def _iou_params(cases):
    return [pytest.param(c, id=L.iou_id(c)) for c in cases]


def test_device_sigmoid_is_exact_at_the_three_logits(mode):
    """the precondition of the exact regime ON THE DEVICE: T = G = 1, N = 8, one logit value each: S = 8 p must be 0, 4, 8"""
    for x, want in zip(L.EXACT_LOGITS, (0.0, 4.0, 8.0)):
        S = run_sums(torch.full((1, 1, 8), x, device="cuda"), torch.ones((1, 1, 8), device="cuda")).cpu()
        assert S.reshape(-1).tolist() == [want, want, 8.0, 0.0], (x, S)


@pytest.mark.parametrize("c", _iou_params(L.IOU_CASES))
def test_softiou_sums_exact(c, mode):
    """every sum EQUALS the float64 count (halves below 2^23), S[:, T, G] stays 0"""
    d = _cached(("iou_exact", L.iou_id(c)), lambda: L.iou_exact_data(c))
    S = run_sums(_dev(d["logits"]), _dev(d["y"]))
    assert_close("S, exact", S, d["S"], 0.0)
    assert float(S[:, c["T"], c["G"]].abs().max()) == 0.0


@pytest.mark.parametrize("c", _iou_params(L.IOU_CASES + L.IOU_BWD_ONLY))
def test_softiou_bwd_exact(c, mode):
    """dlogits EQUALS (ca y + cb (1 - y)) p (1 - p): p (1 - p) in {0, 1/4}, integer ca / cb, perm with repeated slots and perm_ld > T"""
    d = _cached(("iou_exact", L.iou_id(c)), lambda: L.iou_exact_data(c, with_sums=c not in L.IOU_BWD_ONLY))
    got = run_bwd(_dev(d["logits"]), _dev(d["y"]), _dev(d["perm"]), _dev(d["ca"]), _dev(d["cb"]))
    assert_close("dlogits, exact", got, d["dlogits"], 0.0)


def test_softiou_refusals_write_nothing():
    """rsis_softiou_sums refuses (RSIS_ERR_ARG) an empty batch, no prediction, no GT slot, more than 128 of either, N < 8, N % 8 != 0 and
    null pointers at the C ABI, before the launcher's own T = 0 / G = 0 / B = 0 returns can be reached; a refusal leaves S untouched.
    rsis_softiou_bwd: perm_ld < T, N % 4 != 0, null pointers; dlogits untouched."""
    A = _abi()
    Lb = A.lib()
    lg, y = torch.zeros((2, 3, 16), device="cuda"), torch.ones((2, 4, 16), device="cuda")
    S = Guarded((3, 4, 5))
    p, st = A.ptr, A.stream()
    for args in ((p(lg), p(y), p(S.t), 0, 3, 4, 16), (p(lg), p(y), p(S.t), 2, 0, 4, 16), (p(lg), p(y), p(S.t), 2, 3, 0, 16),
                 (p(lg), p(y), p(S.t), 2, 129, 4, 16), (p(lg), p(y), p(S.t), 2, 3, 129, 16), (p(lg), p(y), p(S.t), 2, 3, 4, 4),
                 (p(lg), p(y), p(S.t), 2, 3, 4, 12), (p(lg), p(y), p(S.t), -1, 3, 4, 16), (None, p(y), p(S.t), 2, 3, 4, 16),
                 (p(lg), None, p(S.t), 2, 3, 4, 16), (p(lg), p(y), None, 2, 3, 4, 16)):
        assert Lb.rsis_softiou_sums(*args, st) == ERR_ARG, args[3:]
    torch.cuda.synchronize()
    S.check("S")
    assert S.untouched()
    perm = torch.zeros((2, 5), dtype=torch.int64, device="cuda")
    ca = torch.ones((2, 3), device="cuda")
    dl = Guarded((2, 3, 16))
    for args in ((p(lg), p(y), p(perm), 2, p(ca), p(ca), p(dl.t), 2, 3, 4, 16), (p(lg), p(y), p(perm), 5, p(ca), p(ca), p(dl.t), 2, 3, 4, 14),
                 (p(lg), p(y), p(perm), 5, p(ca), p(ca), p(dl.t), 0, 3, 4, 16), (p(lg), p(y), None, 5, p(ca), p(ca), p(dl.t), 2, 3, 4, 16),
                 (p(lg), p(y), p(perm), 5, None, p(ca), p(dl.t), 2, 3, 4, 16), (p(lg), p(y), p(perm), 5, p(ca), p(ca), None, 2, 3, 4, 16)):
        assert Lb.rsis_softiou_bwd(*args, st) == ERR_ARG, args[3]
    torch.cuda.synchronize()
    dl.check("dlogits")
    assert dl.untouched()


def _iou_normal_params():
    return [pytest.param(c, r, id="%s-%s" % (L.iou_id(c), r)) for c in L.IOU_NORMAL for r in L.IOU_REGIMES]


@pytest.mark.parametrize("c,regime", _iou_normal_params())
def test_softiou_normal(c, regime, mode):
    """sums within M_IOU * err_host; the all-pairs cost and the matched cost within the bar propagated through 1 - I / U (module
    docstring); dlogits within K_DLOGITS roundings, relative plus absolute against the larger coefficient of the row"""
    from rsis_amd import ops
    d = _cached(("iou_normal", L.iou_id(c), regime), lambda: L.iou_normal_data(c, regime))
    B, T, G = c["B"], c["T"], c["G"]
    lg, y, perm = _dev(d["logits"]), _dev(d["y"]), _dev(d["perm"])
    S = run_sums(lg, y)
    err_gpu = _max_err(S, d["S"])
    _record("iou", "%s-%s" % (L.iou_id(c), regime), mode, d["err_host"], err_gpu)
    E = L.M_IOU * d["err_host"]
    assert err_gpu <= E, "sums: err_gpu %.3e > %.2f * err_host %.3e" % (err_gpu, L.M_IOU, d["err_host"])
    assert float(S[:, T, G].abs().max()) == 0.0
    bar = 4 * E / d["den"] + 8 * U24                                      # (B, G, T)
    cost = ops.softiou_cost_matrix(S).double().cpu().numpy()
    over = np.abs(cost - d["cost"]) - bar
    assert over.max() <= 0, "cost: %.3e over the bar at %s" % (over.max(), np.unravel_index(over.argmax(), over.shape))
    matched = ops.softiou_matched(lg, y, perm, S).double().cpu().numpy()    # (B, T): the pair (perm[b, t], t)
    bi, ti = np.arange(B)[:, None], np.arange(T)[None, :]
    gi = d["perm"][:, :T]
    over = np.abs(matched - d["cost"][bi, gi, ti]) - bar[bi, gi, ti]
    assert over.max() <= 0, "matched cost: %.3e over the bar" % over.max()
    got = run_bwd(lg, y, perm, _dev(d["ca"]), _dev(d["cb"])).double().cpu().numpy()
    coef = np.maximum(np.abs(d["ca"]), np.abs(d["cb"])).astype(np.float64)[:, :, None]
    over = np.abs(got - d["dlogits"]) - L.K_DLOGITS * U24 * (np.abs(d["dlogits"]) + coef)
    assert over.max() <= 0, "dlogits: %.3e over %d roundings at %s" % (over.max(), L.K_DLOGITS, np.unravel_index(over.argmax(), over.shape))


# ======================================================================================================================
# 2. heads
# ======================================================================================================================
def run_heads_fwd(sides, Wc, bc, Ws, bs):
    A = _abi()
    rows, ncls = sides[0].shape[0], Wc.shape[0]
    probs, stop = Guarded((rows, ncls)), Guarded((rows,))
    A.check(A.lib().rsis_heads_fwd(A.ptr_array(sides), A.int_array([s.shape[1] for s in sides]), len(sides), rows, A.ptr(Wc), A.ptr(bc), ncls,
                                   A.ptr(Ws), A.ptr(bs), A.ptr(probs.t), A.ptr(stop.t), A.stream()), "rsis_heads_fwd")
    torch.cuda.synchronize()
    probs.check("probs"), stop.check("stop")
    return probs.t, stop.t


class HeadsBwd(object):
    """device operands and guarded outputs of rsis_heads_bwd calls on one case; `null` names the pointers passed as NULL:
    dprobs, dstop, dside<i>, dWc, dbc, dWs, dbs.  The parameter gradients start from `fill` (zeros where None)."""

    def __init__(self, d, fill=None, null=()):
        self.d, self.null = d, set(null)
        self.sides = [_dev(s) for s in d["sides"]]
        self.Cs = [s.shape[1] for s in d["sides"]]
        self.rows = d["sides"][0].shape[0]
        self.Wc, self.Ws = _dev(d["Wc"]), _dev(d["Ws"])
        self.ncls = d["Wc"].shape[0]
        self.probs = _dev(d.get("probs_in", d.get("probs")))
        self.dprobs, self.dstop = _dev(d["dprobs"]), _dev(d["dstop"])
        self.dside = [Guarded((self.rows, c)) for c in self.Cs]
        shapes = dict(dWc=d["Wc"].shape, dbc=(self.ncls,), dWs=d["Ws"].shape, dbs=(1,))
        self.fill = {k: (fill[k] if fill is not None else np.zeros(sh, np.float32)) for k, sh in shapes.items()}
        self.par = {k: Guarded(sh, init=_t(self.fill[k])) for k, sh in shapes.items()}

    def call(self, rows=None, row0=0):
        """one launch over `rows` rows starting at row0 (default: all); returns the status"""
        A = _abi()
        rows = self.rows if rows is None else rows
        sl = slice(row0, row0 + rows)
        po = lambda name, t: None if name in self.null else A.ptr(t)
        dsides = [None if "dside%d" % i in self.null else g.t[sl] for i, g in enumerate(self.dside)]
        rc = A.lib().rsis_heads_bwd(A.ptr_array([s[sl] for s in self.sides]), A.int_array(self.Cs), len(self.Cs), rows, A.ptr(self.Wc), self.ncls,
                                    A.ptr(self.Ws), A.ptr(self.probs[sl]), po("dprobs", self.dprobs[sl]), po("dstop", self.dstop[sl]),
                                    A.ptr_array(dsides), po("dWc", self.par["dWc"].t), po("dbc", self.par["dbc"].t), po("dWs", self.par["dWs"].t),
                                    po("dbs", self.par["dbs"].t), A.stream())
        torch.cuda.synchronize()
        for i, g in enumerate(self.dside):
            g.check("dside[%d]" % i)
        for k, g in self.par.items():
            g.check(k)
        return rc

    def compare(self, ref, what, atol=0.0):
        """d side and the parameter gradients (on top of the fill) against `ref`; a NULL output must still hold its initial contents"""
        off = 0
        for i, (g, c) in enumerate(zip(self.dside, self.Cs)):
            if "dside%d" % i in self.null:
                assert g.untouched(), "%s: dside[%d] was passed as NULL and written" % (what, i)
            else:
                assert_close("%s: dside[%d]" % (what, i), g.t, ref["dside"][:, off:off + c], atol)
            off += c
        for k, g in self.par.items():
            want = self.fill[k].astype(np.float64) + (0.0 if k in self.null else ref[k].reshape(self.fill[k].shape))
            assert_close("%s: %s" % (what, k), g.t, want, 0.0 if k in self.null else atol)


def _heads_params(shapes):
    return [pytest.param(s, id=L.heads_id(s)) for s in shapes]


@pytest.mark.parametrize("s", _heads_params(L.HEADS_SHAPES))
def test_heads_fwd_stop_exact(s, mode):
    """integer features and weights: the stop logit EQUALS float64; the class probabilities are a distribution"""
    d = _cached(("heads_exact", L.heads_id(s)), lambda: L.heads_exact_data(s))
    probs, stop = run_heads_fwd([_dev(a) for a in d["sides"]], _dev(d["Wc"]), _dev(d["bc"]), _dev(d["Ws"]), _dev(d["bs"]))
    assert_close("stop, exact", stop, d["stop"], 0.0)
    p = probs.double().cpu()
    assert bool((p >= 0).all()) and float((p.sum(1) - 1).abs().max()) <= (s[2] + 2) * U24


@pytest.mark.parametrize("s", _heads_params(L.HEADS_BWD_EXACT))
def test_heads_bwd_exact(s, mode):
    """probs 1 / 2^k, integer dprobs / dstop, integer non-zero prefill: d side and every gradient on top of its prefill EQUAL float64"""
    d = _cached(("heads_exact", L.heads_id(s)), lambda: L.heads_exact_data(s))
    h = HeadsBwd(d, d["fill"])
    assert h.call() == OK
    h.compare(d["ref"], "exact")


@pytest.mark.parametrize("null", [("dprobs",), ("dstop",), ("dside1",), ("dWc",), ("dWs",), ("dWc", "dbc", "dWs", "dbs"), ("dside0", "dside1", "dside2", "dside3", "dside4")],
                         ids=lambda n: "+".join(n) if len(n) < 3 else n[0] + "..")
def test_heads_bwd_null_pointers(null):
    """a NULL gradient input counts as zero, a NULL output is skipped: everything else still EQUALS float64 on top of its prefill"""
    s = L.HEADS_SHAPES[5]
    d = _cached(("heads_exact", L.heads_id(s)), lambda: L.heads_exact_data(s))
    ref = L.heads_bwd64(d["sides"], d["Wc"], d["Ws"], d["probs"], None if "dprobs" in null else d["dprobs"], None if "dstop" in null else d["dstop"])
    h = HeadsBwd(d, d["fill"], null)
    assert h.call() == OK
    h.compare(ref, "null " + "+".join(null))


def _limit_case(rows):
    Cs, ncls = L.HEADS_LIMIT
    return (rows, Cs, ncls)


def test_heads_bwd_lds_limit():
    """ncls 21, K 248: 364 rows are the most that fit 64 KB of LDS (succeeds, EQUALS float64); 365 are refused with RSIS_ERR_UNSUPPORTED
    and every output buffer still at its fill"""
    fits, refused = L.heads_max_rows(sum(L.HEADS_LIMIT[0]), L.HEADS_LIMIT[1])
    d = _cached(("heads_exact", fits), lambda: L.heads_exact_data(_limit_case(fits)))
    h = HeadsBwd(d, d["fill"])
    assert h.call() == OK
    h.compare(d["ref"], "%d rows" % fits)
    d = L.heads_exact_data(_limit_case(refused))
    h = HeadsBwd(d, d["fill"])
    assert h.call() == UNSUPPORTED
    assert all(g.untouched() for g in h.dside), "a refused call wrote d side"
    for k, g in h.par.items():
        assert_close("refused: %s" % k, g.t, h.fill[k], 0.0)


@pytest.mark.parametrize("regime", ["exact", "normal"])
def test_heads_bwd_one_launch_equals_per_step_launches(regime):
    """T * B = 28 * 13 = 364 rows in ONE launch against 28 launches of 13 rows that accumulate into the same parameter gradients (the two
    forms of decoder_seq._heads_bwd_all_steps): d side equal by BITS; the parameter sums equal by bits on exact data and, on normal data,
    within the bound of two fp32 summations of the same n = 364 terms in different orders, 2 (n - 1) 2^-24 sum |terms|"""
    T, B = 28, 13
    s = _limit_case(T * B)
    d = _cached(("heads_exact", T * B), lambda: L.heads_exact_data(s)) if regime == "exact" else L.heads_normal_data(s, "normal")
    one, steps = HeadsBwd(d, d.get("fill")), HeadsBwd(d, d.get("fill"))
    assert one.call() == OK
    for t in range(T):
        assert steps.call(B, t * B) == OK
    for i, (a, b) in enumerate(zip(one.dside, steps.dside)):
        assert torch.equal(a.t, b.t), "dside[%d]" % i
    if regime == "exact":
        steps.compare(d["ref"], "per step")
        for k in one.par:
            assert torch.equal(one.par[k].t, steps.par[k].t), k
        return
    dl = np.concatenate([np.abs(d["ref"]["dl"]), np.abs(d["dstop"]).astype(np.float64)[:, None]], 1)          # (rows, ncls + 1)
    sv = np.abs(np.concatenate(d["sides"], 1)).astype(np.float64)
    bound = 2 * (T * B - 1) * U24
    ncls = s[2]
    for k, mag in (("dWc", dl[:, :ncls].T @ sv), ("dWs", dl[:, ncls] @ sv), ("dbc", dl[:, :ncls].sum(0)), ("dbs", dl[:, ncls:].sum(0))):
        diff = (one.par[k].t.double() - steps.par[k].t.double()).abs().cpu().numpy()
        assert (diff <= bound * mag.reshape(diff.shape)).all(), "%s: one launch and %d launches differ by %.3e" % (k, T, diff.max())
        assert_close("%s against float64" % k, one.par[k].t, d["ref"][k].reshape(diff.shape), float((bound * mag).max()))


@pytest.mark.parametrize("T,B", [(28, 13), (28, 14)], ids=["364_rows_one_launch", "392_rows_per_step"])
def test_decoder_seq_heads_bwd_falls_back_per_step(T, B):
    """decoder_seq._heads_bwd_all_steps: 392 rows do not fit the kernel's LDS (status 3), so the T steps are launched one by one; both
    forms EQUAL float64 on exact data"""
    from rsis_amd import decoder_seq
    A = _abi()
    s = _limit_case(T * B)
    assert L.heads_fits(T * B, sum(s[1]), s[2]) == (B == 13)
    d = L.heads_exact_data(s)
    h = HeadsBwd(d, d["fill"])
    tb = lambda t, c: t.view(T, B, c) if c else t.view(T, B)
    levels = [types.SimpleNamespace(SIDE=tb(sd, c)) for sd, c in zip(h.sides, h.Cs)]
    decoder_seq._heads_bwd_all_steps(A.lib(), levels, h.Cs, len(h.Cs), T, B, h.Wc, h.Ws, tb(h.probs, h.ncls), tb(h.dprobs, h.ncls), tb(h.dstop, 0),
                                     [tb(g.t, c) for g, c in zip(h.dside, h.Cs)], [h.par[k].t for k in ("dWc", "dbc", "dWs", "dbs")])
    torch.cuda.synchronize()
    for g in h.dside + list(h.par.values()):
        g.check("heads backward of all steps")
    h.compare(d["ref"], "%d x %d rows" % (T, B))


@pytest.mark.parametrize("regime", ["normal", "hot"])
@pytest.mark.parametrize("s", _heads_params(L.HEADS_NORMAL))
def test_heads_normal(s, regime, mode):
    """probs, stop, d side and the parameter gradients within M_HEADS * err_host of float64, err_host per output group"""
    d = _cached(("heads_normal", L.heads_id(s), regime), lambda: L.heads_normal_data(s, regime))
    probs, stop = run_heads_fwd([_dev(a) for a in d["sides"]], _dev(d["Wc"]), _dev(d["bc"]), _dev(d["Ws"]), _dev(d["bs"]))
    h = HeadsBwd(d)
    assert h.call() == OK
    ref = d["ref"]
    dside = torch.cat([g.t for g in h.dside], 1)
    err = dict(probs=_max_err(probs, d["probs"]), stop=_max_err(stop, d["stop"]), dside=_max_err(dside, ref["dside"]),
               params=max(_max_err(h.par[k].t, ref[k].reshape(h.fill[k].shape)) for k in h.par))
    bad = []
    for k in ("probs", "stop", "dside", "params"):
        _record("heads", "%s-%s-%s" % (L.heads_id(s), regime, k), mode, d["err_host"][k], err[k])
        if not err[k] <= L.M_HEADS * d["err_host"][k]:
            bad.append("%s: err_gpu %.3e > %.2f * err_host %.3e" % (k, err[k], L.M_HEADS, d["err_host"][k]))
    assert not bad, "; ".join(bad)


def test_heads_fwd_keys_decodes_chosen_keys(mode):
    """rsis_heads_fwd_keys on keys built by the Python restatement of rsis_side_key for +-0.0, negative normals, +-FLT_MAX, denormals and
    the pixels 0 and 2^20 - 1: side_out has the BITS of the value, arg_out the pixel, and probs / stop the bits rsis_heads_fwd gives on
    the decoded features"""
    A = _abi()
    d = L.keys_data()
    rows, Cs, ncls = L.KEYS_SHAPE
    keys = [_t(k.view(np.int64)).cuda() for k in d["keys"]]
    side_out, arg_out = [Guarded((rows, c)) for c in Cs], [GuardedInt((rows, c), torch.int32) for c in Cs]
    probs, stop = Guarded((rows, ncls)), Guarded((rows,))
    Wc, bc, Ws, bs = (_dev(d[k]) for k in ("Wc", "bc", "Ws", "bs"))
    A.check(A.lib().rsis_heads_fwd_keys(A.ptr_array(keys), A.ptr_array([g.t for g in side_out]), A.ptr_array([g.t for g in arg_out]), A.int_array(Cs),
                                        len(Cs), rows, A.ptr(Wc), A.ptr(bc), ncls, A.ptr(Ws), A.ptr(bs), A.ptr(probs.t), A.ptr(stop.t), A.stream()),
            "rsis_heads_fwd_keys")
    torch.cuda.synchronize()
    for i, (so, ao) in enumerate(zip(side_out, arg_out)):
        so.check("side_out[%d]" % i), ao.check("arg_out[%d]" % i)
        assert np.array_equal(so.t.cpu().numpy().view(np.uint32), d["vals"][i].view(np.uint32)), "side_out[%d]: not the bits of the value" % i
        assert np.array_equal(ao.t.cpu().numpy(), d["pix"][i]), "arg_out[%d]" % i
    probs.check("probs"), stop.check("stop")
    p2, s2 = run_heads_fwd([_dev(v) for v in d["vals"]], Wc, bc, Ws, bs)
    assert torch.equal(probs.t.view(torch.int32), p2.view(torch.int32)) and torch.equal(stop.t.view(torch.int32), s2.view(torch.int32))
    assert bool(torch.isfinite(probs.t).all()) and bool(torch.isfinite(stop.t).all())


# ======================================================================================================================
# 3. loss tail
# ======================================================================================================================
def run_tail(q):
    """the two calls of ops._LossTailFn: forward (out only), backward (gradients only); returns out[4], dprobs, dstop, dsiou"""
    A = _abi()
    n, C = q["probs"].shape
    probs, y, stop, siou, swm, swc, cw = (_dev(q[k]) for k in ("probs", "y", "stop", "siou", "swm", "swc", "cw"))
    gout = torch.tensor([float(q["gout"])], device="cuda") if q["gout"] is not None else None
    bw = float(q["bw"]) if q["bw"] is not None else -1.0
    w = [float(v) for v in L.TAIL_W]
    out, dprobs, dstop, dsiou = Guarded((4,)), Guarded((n, C)), Guarded((n,)), Guarded((n,))
    common = (A.ptr(probs), A.ptr(y), A.ptr(stop), A.ptr(siou), A.ptr(swm), A.ptr(swc), A.ptr(cw), n, C, bw, w[0], w[1], w[2])
    A.check(A.lib().rsis_loss_tail(*common, A.ptr(out.t), None, None, None, None, A.stream()), "rsis_loss_tail")
    A.check(A.lib().rsis_loss_tail(*common, None, A.ptr(dprobs.t), A.ptr(dstop.t), A.ptr(dsiou.t), A.ptr(gout), A.stream()), "rsis_loss_tail(bwd)")
    torch.cuda.synchronize()
    for g, nm in ((out, "out"), (dprobs, "dprobs"), (dstop, "dstop"), (dsiou, "dsiou")):
        g.check(nm)
    return out.t, dprobs.t, dstop.t, dsiou.t


@pytest.mark.parametrize("c", [pytest.param(c, id=L.tail_id(c)) for c in L.TAIL_CASES])
def test_loss_tail(c):
    """total and the three means within M_TAIL * err_host (the largest error of the four against the host model's); dsiou, dprobs, dstop
    elementwise within K_DSIOU, K_DPROBS, K_DSTOP roundings (dstop: plus the same count absolute against its coefficient); the gradients
    of unselected rows are exactly 0 (their reference is 0 and the bar is relative).

    M_TAIL is the cap of 4, not twice a measured ratio (MI355X, profiles/r14_a_loss_path_margins.txt):
      n320_c21_auto_cw_normal, n320_c64_auto_cw_normal   ratios 3.73 and 3.22, every other case <= 1.52.  Both are the class NLL mean: the
                             host chain landed 0.3 ulp from float64 there (7.0e-8 at a mean of ~3), the kernel's strided partials and tree
                             1.7 and 1.2 ulp (4.07e-7, 5.83e-7).  Four scalars per case are single draws, not a maximum over a population,
                             so such ratios say nothing about the 256-stride loops -- a skipped or doubled row moves a mean by ~1e-3.
      n1_c21_auto_nocw_hot   found a weakness: with -logf(p) the one-row class loss -log(1e-30) = 69.0775528 came back one ulp high
                             (7.6e-6, logf's documented accuracy; ratio 78).  loss_tail_kernel takes this log in fp64 and rounds once
                             since: err_gpu = err_host = 9.762e-08."""
    q = L.tail_inputs(c)
    r, h = L.tail_eval(q, np.float64), L.tail_eval(q, np.float32)
    out, dprobs, dstop, dsiou = run_tail(q)
    err_host, err_gpu = float(np.abs(h["out"].astype(np.float64) - r["out"]).max()), _max_err(out, r["out"])
    _record("tail", L.tail_id(c), "-", err_host, err_gpu)
    print("       (total, iou, stop, class): host %s  gpu %s" % (np.abs(h["out"].astype(np.float64) - r["out"]), np.abs(out.double().cpu().numpy() - r["out"])))
    assert err_gpu <= L.M_TAIL * err_host, "out %s against %s: err_gpu %.3e > %.2f * err_host %.3e" % (out.tolist(), r["out"].tolist(), err_gpu, L.M_TAIL, err_host)
    for nm, got, k, extra in (("dsiou", dsiou, L.K_DSIOU, 0.0), ("dprobs", dprobs, L.K_DPROBS, 0.0), ("dstop", dstop, L.K_DSTOP, r["coef"])):
        g = got.double().cpu().numpy()
        assert np.isfinite(g).all(), nm
        over = np.abs(g - r[nm]) - k * U24 * (np.abs(r[nm]) + extra)
        assert over.max() <= 0, "%s: %.3e over %d roundings at %s" % (nm, over.max(), k, np.unravel_index(over.argmax(), over.shape))
    sel_m, sel_c = q["swm"] > 0, q["swc"] > 0
    assert not dprobs[_t(~sel_m).cuda()].any() and not dsiou[_t(~sel_m).cuda()].any() and not dstop[_t(~sel_c).cuda()].any()


@pytest.mark.parametrize("n", L.TAIL_MASKING_N)
def test_loss_tail_unselected_rows_never_enter(n):
    """probability 0 at the target class in every row with sw_mask = 0 and a NaN stop logit in every row with sw_class = 0: totals, parts
    and gradients are finite, BIT-EQUAL to the call with benign values in those rows, and exactly 0 in those rows"""
    c = dict(n=n, C=21, bw=False, cw=True, regime="normal", gout=True)
    q = L.tail_inputs(c)
    bad = dict(q, probs=q["probs"].copy(), stop=q["stop"].copy())
    um, uc = np.flatnonzero(q["swm"] == 0), np.flatnonzero(q["swc"] == 0)
    assert um.size and uc.size
    bad["probs"][um, q["y"][um]] = 0.0
    bad["stop"][uc] = np.nan
    good, poisoned = run_tail(q), run_tail(bad)
    for nm, a, b in zip(("out", "dprobs", "dstop", "dsiou"), good, poisoned):
        assert bool(torch.isfinite(b).all()), "%s is not finite" % nm
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s changed with the contents of unselected rows" % nm
    _, dprobs, dstop, dsiou = poisoned
    assert not dprobs[_t(um).cuda()].any() and not dsiou[_t(um).cuda()].any() and not dstop[_t(uc).cuda()].any()
    r = L.tail_eval(q, np.float64)
    assert _max_err(poisoned[0], r["out"]) <= L.M_TAIL * float(np.abs(L.tail_eval(q, np.float32)["out"].astype(np.float64) - r["out"]).max())


# ======================================================================================================================
# 4. assignment
# ======================================================================================================================
@pytest.mark.parametrize("struct", L.ASSIGN_STRUCTS)
@pytest.mark.parametrize("G,T", L.ASSIGN_SIZES, ids=["g%d_t%d" % s for s in L.ASSIGN_SIZES])
def test_assignment_is_optimal_under_ties(G, T, struct):
    """quantised scores (the float64 total of any assignment is exact): the T matched slots are distinct, perm[:, T:] is 0, the total of
    the device's assignment EQUALS scipy's optimum, and a second call gives the same bits.  Which of several tied optima comes back is
    pinned too: perm EQUALS the sequential float64 run of the same algorithm, whose scan keeps the first minimum (exact potentials, so
    there is no rounding to excuse a difference).  G <= 64: assign_kernel (arg-min, smallest lane on ties); G >= 65: assign2_kernel
    (ballot / ffs, column < 64 first)."""
    A = _abi()
    s = L.assign_scores(G, T, struct)
    sd = _dev(s)
    perms = []
    for _ in range(2):
        perm = GuardedInt((L.ASSIGN_B, G), torch.int64)
        A.check(A.lib().rsis_assign_min_cost(A.ptr(sd), A.ptr(perm.t), L.ASSIGN_B, G, T, A.stream()), "rsis_assign_min_cost")
        torch.cuda.synchronize()
        perm.check("perm")
        perms.append(perm.t.cpu().numpy())
    p = perms[0]
    assert np.array_equal(p, perms[1]), "two calls differ"
    assert p.min() >= 0 and p.max() < G
    for b in range(L.ASSIGN_B):
        assert len(set(p[b, :T].tolist())) == T, "image %d: not an assignment: %s" % (b, p[b, :T])
    assert not p[:, T:].any(), "perm[:, T:] must be 0"
    got, best = L.assign_total(s, p), L.assign_optimum(s)
    assert np.array_equal(got, best), "totals %s against the optimum %s" % (got, best)
    want = L.assign_sequential(s)
    assert np.array_equal(p, want), "not the optimum the sequential scan reaches: image %d" % int(np.flatnonzero((p != want).any(1))[0])
