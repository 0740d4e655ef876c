"""rsis_softiou_sums_ignore / rsis_softiou_bwd_ignore (csrc/losses.hip) against the FLOAT64 statement of softiou_ignore_cases.py, through
the C ABI, in the default and in the deterministic mode, with the regimes and bars of test_gpu_loss_path.py:

  * EXACT: logits from {-100, 0, +30}, masks in {0, 1}: every sum is a count in halves, dlogits a small dyadic: EQUALITY with float64;
  * NORMAL: N(0, 2) and N(0, 12): sums within M_IOU_IGN * err_host (err_host: the fp32 sequential chain over the masked terms), costs
    within 4 E / U + 8 * 2^-24, dlogits within K_DLOGITS roundings (the factor k is exact: the derivation of loss_path_cases.py holds);
  * properties of the map: +0.0 by bits under every ignored pixel; ignored logits have no influence; an all-zero map and a NULL map give
    the bits of the plain entry points; an all-ones map gives cost 1.0f for every pair.

Every output is a guarded view.  One line per normal case is printed (RSIS_IGNORE_MARGINS=<file>: appended there: the margin survey)."""
import os

import numpy as np
import pytest
import torch

import loss_path_cases as L
import softiou_ignore_cases as C
from helpers import Guarded, assert_close, to_tensor as _t

pytestmark = pytest.mark.gpu
U24 = L.U24
ERR_ARG = 1


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


def _dev(a):
    return _t(a).cuda()


def _abi():
    from rsis_amd import _lib
    return _lib


def run_sums(logits, y, ignore):
    """ignore None: a NULL map"""
    A = _abi()
    B, T, N = logits.shape
    G = y.shape[1]
    S = Guarded((B, T + 1, G + 1))
    A.check(A.lib().rsis_softiou_sums_ignore(A.ptr(logits), A.ptr(y), A.ptr(ignore) if ignore is not None else None, A.ptr(S.t), B, T, G, N,
                                             A.stream()), "rsis_softiou_sums_ignore")
    torch.cuda.synchronize()
    S.check("S")
    return S.t


def run_bwd(logits, y, ignore, perm, ca, cb):
    A = _abi()
    B, T, N = logits.shape
    d = Guarded((B, T, N))
    A.check(A.lib().rsis_softiou_bwd_ignore(A.ptr(logits), A.ptr(y), A.ptr(ignore) if ignore is not None else None, A.ptr(perm), perm.shape[1],
                                            A.ptr(ca), A.ptr(cb), A.ptr(d.t), B, T, y.shape[1], N, A.stream()), "rsis_softiou_bwd_ignore")
    torch.cuda.synchronize()
    d.check("dlogits")
    return d.t


def run_plain(logits, y, perm=None, ca=None, cb=None):
    """the plain entry points: S, or dlogits when perm is given"""
    A = _abi()
    B, T, N = logits.shape
    G = y.shape[1]
    if perm is None:
        S = Guarded((B, T + 1, G + 1))
        A.check(A.lib().rsis_softiou_sums(A.ptr(logits), A.ptr(y), A.ptr(S.t), B, T, G, N, A.stream()), "rsis_softiou_sums")
        torch.cuda.synchronize()
        return S.t
    d = Guarded((B, T, N))
    A.check(A.lib().rsis_softiou_bwd(A.ptr(logits), A.ptr(y), A.ptr(perm), perm.shape[1], A.ptr(ca), A.ptr(cb), A.ptr(d.t), B, T, G, N,
                                     A.stream()), "rsis_softiou_bwd")
    torch.cuda.synchronize()
    return d.t


_DATA = {}


def _cached(key, build):
    """host inputs and float64 references of a case, computed once and shared by the modes (never modified)"""
    if key not in _DATA:
        _DATA[key] = build()
    return _DATA[key]


def _params(cases, patterns=C.PATTERNS):
    return [pytest.param(c, p, id="%s-%s" % (L.iou_id(c), p)) for c in cases for p in patterns]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _zero_bits_under_ignore(dl, ignore):
    """dlogits is +0.0, by bits, at every ignored pixel of every prediction"""
    ig = (ignore != 0).unsqueeze(1).expand_as(dl)
    assert int((_bits(dl)[ig] != 0).sum()) == 0, "dlogits: non-zero bits under ignored pixels"


# ---------------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("c,pattern", _params(C.IGN_CASES))
def test_sums_exact(c, pattern, mode):
    """every sum EQUALS the float64 count over the kept pixels; S[:, T, G] stays 0"""
    d = _cached(("exact", L.iou_id(c), pattern), lambda: C.exact_data(c, pattern))
    S = run_sums(_dev(d["logits"]), _dev(d["y"]), _dev(d["ignore"]))
    assert_close("S, exact", S, d["S"], 0.0)
    assert float(S[:, c["T"], c["G"]].abs().max()) == 0.0


@pytest.mark.parametrize("c,pattern", _params(C.IGN_CASES + C.IGN_BWD_ONLY))
def test_bwd_exact(c, pattern, mode):
    """dlogits EQUALS k (ca y + cb (1 - y)) p (1 - p), and is +0.0 by bits under the map"""
    d = _cached(("exact", L.iou_id(c), pattern), lambda: C.exact_data(c, pattern, with_sums=c not in C.IGN_BWD_ONLY))
    ign = _dev(d["ignore"])
    got = run_bwd(_dev(d["logits"]), _dev(d["y"]), ign, _dev(d["perm"]), _dev(d["ca"]), _dev(d["cb"]))
    assert_close("dlogits, exact", got, d["dlogits"], 0.0)
    _zero_bits_under_ignore(got, ign)


# ---------------------------------------------------------------------------------------------------------------------- normal
def _record(cid, mode, err_host, err_gpu):
    ratio = err_gpu / err_host if err_host > 0 else (0.0 if err_gpu == 0 else float("inf"))
    line = "iou-ign %-44s %-13s err_host %.3e  err_gpu %.3e  ratio %.3f" % (cid, mode, err_host, err_gpu, ratio)
    print(line)
    if os.environ.get("RSIS_IGNORE_MARGINS"):
        with open(os.environ["RSIS_IGNORE_MARGINS"], "a") as f:
            f.write(line + "\n")


def _normal_params():
    return [pytest.param(c, r, p, id="%s-%s-%s" % (L.iou_id(c), r, p)) for c in C.IGN_NORMAL for r in L.IOU_REGIMES for p in C.PATTERNS]


@pytest.mark.parametrize("c,regime,pattern", _normal_params())
def test_normal(c, regime, pattern, mode):
    """sums within M_IOU_IGN * err_host; all-pairs cost within 4 E / U + 8 u; dlogits within K_DLOGITS roundings and +0.0 under the map"""
    from rsis_amd import ops
    d = _cached(("normal", L.iou_id(c), regime, pattern), lambda: C.normal_data(c, regime, pattern))
    T, G = c["T"], c["G"]
    lg, y, ign, perm = _dev(d["logits"]), _dev(d["y"]), _dev(d["ignore"]), _dev(d["perm"])
    S = run_sums(lg, y, ign)
    err_gpu = float(np.abs(S.double().cpu().numpy() - d["S"]).max())
    _record("%s-%s-%s" % (L.iou_id(c), regime, pattern), mode, d["err_host"], err_gpu)
    E = C.M_IOU_IGN * d["err_host"]
    assert err_gpu <= E, "sums: err_gpu %.3e > %.2f * err_host %.3e" % (err_gpu, C.M_IOU_IGN, d["err_host"])
    assert float(S[:, T, G].abs().max()) == 0.0
    bar = 4 * E / d["den"] + 8 * U24                                      # (B, G, T)
    cost = ops.softiou_cost_matrix(S).double().cpu().numpy()
    over = np.abs(cost - d["cost"]) - bar
    assert over.max() <= 0, "cost: %.3e over the bar at %s" % (over.max(), np.unravel_index(over.argmax(), over.shape))
    matched = ops.softiou_matched(lg, y, perm, S, ignore=ign).double().cpu().numpy()    # (B, T): the pair (perm[b, t], t)
    bi, ti = np.arange(c["B"])[:, None], np.arange(T)[None, :]
    gi = d["perm"][:, :T]
    over = np.abs(matched - d["cost"][bi, gi, ti]) - bar[bi, gi, ti]
    assert over.max() <= 0, "matched cost: %.3e over the bar" % over.max()
    got_t = run_bwd(lg, y, ign, perm, _dev(d["ca"]), _dev(d["cb"]))
    _zero_bits_under_ignore(got_t, ign)
    got = got_t.double().cpu().numpy()
    coef = np.maximum(np.abs(d["ca"]), np.abs(d["cb"])).astype(np.float64)[:, :, None]
    over = np.abs(got - d["dlogits"]) - L.K_DLOGITS * U24 * (np.abs(d["dlogits"]) + coef)
    assert over.max() <= 0, "dlogits: %.3e over %d roundings at %s" % (over.max(), L.K_DLOGITS, np.unravel_index(over.argmax(), over.shape))


_SMALL = [c for c in C.IGN_CASES if c not in C.IGN_NORMAL]         # b2_t1_g1_n8, b2_t32_g1_n64, b2_t1_g32_n64


@pytest.mark.parametrize("c,regime,pattern", [pytest.param(c, r, p, id="%s-%s-%s" % (L.iou_id(c), r, p))
                                              for c in _SMALL for r in L.IOU_REGIMES for p in C.PATTERNS])
def test_normal_small_shapes(c, regime, pattern, mode):
    """The smallest ones-row and tiled shapes under N(0, 2) and N(0, 12).  Their sums have too few terms for the err_host yardstick
    (loss_path_cases.MIN_TERMS), so the bar is a priori: every term is >= 0, the fp32 sigmoid and the product are within 5 u, and ANY
    order of N - 1 rounded fp32 additions of non-negative terms stays within (N - 1) u of the sum: e = (N + 4) u relative, taken twice
    (the MFMA's own accumulation is not documented to round to nearest).  Sums within 2 e S; |d(I / U)| <= e' I / U + 3 e' I / U <= 4 e'
    with e' = 2 e, so costs within 8 e + 8 u; dlogits within K_DLOGITS roundings and +0.0 under the map, as everywhere."""
    from rsis_amd import ops
    d = _cached(("normal", L.iou_id(c), regime, pattern), lambda: C.normal_data(c, regime, pattern))
    T, G, N = c["T"], c["G"], c["N"]
    e2 = 2 * (N + 4) * U24
    lg, y, ign, perm = _dev(d["logits"]), _dev(d["y"]), _dev(d["ignore"]), _dev(d["perm"])
    S = run_sums(lg, y, ign)
    over = np.abs(S.double().cpu().numpy() - d["S"]) - e2 * d["S"] - N * 2.0 ** -126      # (+ N underflows: a sigmoid below fp32's normal range)
    assert over.max() <= 0, "sums: %.3e over the a-priori bar" % over.max()
    assert float(S[:, T, G].abs().max()) == 0.0
    cost = ops.softiou_cost_matrix(S).double().cpu().numpy()
    over = np.abs(cost - d["cost"]) - (4 * e2 + 8 * U24)
    assert over.max() <= 0, "cost: %.3e over the bar" % over.max()
    got_t = run_bwd(lg, y, ign, perm, _dev(d["ca"]), _dev(d["cb"]))
    _zero_bits_under_ignore(got_t, ign)
    coef = np.maximum(np.abs(d["ca"]), np.abs(d["cb"])).astype(np.float64)[:, :, None]
    over = np.abs(got_t.double().cpu().numpy() - d["dlogits"]) - L.K_DLOGITS * U24 * (np.abs(d["dlogits"]) + coef)
    assert over.max() <= 0, "dlogits: %.3e over %d roundings" % (over.max(), L.K_DLOGITS)


# ---------------------------------------------------------------------------------------------------------------------- the map
_PROP_CASES = [c for c in C.IGN_CASES if L.iou_id(c) in ("b3_t10_g20_n4096", "b2_t31_g5_n72", "b1_t33_g33_n520", "b1_t65_g127_n136",
                                                         "b1_t128_g128_n520")]


@pytest.mark.parametrize("c", [pytest.param(c, id=L.iou_id(c)) for c in _PROP_CASES])
def test_ignored_logits_have_no_influence(c, deterministic):
    """deterministic mode: other finite logits under the ignored pixels (huge, negative, denormal) change no bit of S"""
    d = _cached(("normal", L.iou_id(c), "n2", "p30"), lambda: C.normal_data(c, "n2", "p30"))
    lg, y, ign = _dev(d["logits"]), _dev(d["y"]), _dev(d["ignore"])
    S0 = run_sums(lg, y, ign).clone()
    other = torch.tensor([3.0e38, -3.0e38, 1e-40, 88.0, -17.5], device="cuda")[torch.arange(lg.numel(), device="cuda") % 5].view_as(lg)
    lg2 = torch.where((ign != 0).unsqueeze(1).expand_as(lg), other, lg)
    assert not torch.equal(lg2, lg)
    S1 = run_sums(lg2, y, ign)
    assert torch.equal(_bits(S0), _bits(S1))


@pytest.mark.parametrize("c", [pytest.param(c, id=L.iou_id(c)) for c in C.IGN_CASES])
def test_zero_map_is_the_plain_entry_point(c, deterministic):
    """deterministic mode, all-zero map: S and dlogits bit-equal to rsis_softiou_sums / rsis_softiou_bwd"""
    d = _cached(("normal", L.iou_id(c), "n2", "zero"), lambda: C.normal_data(c, "n2", "zero"))
    lg, y, ign, perm, ca, cb = (_dev(d[k]) for k in ("logits", "y", "ignore", "perm", "ca", "cb"))
    assert int(ign.sum()) == 0
    assert torch.equal(_bits(run_sums(lg, y, ign)), _bits(run_plain(lg, y)))
    assert torch.equal(_bits(run_bwd(lg, y, ign, perm, ca, cb)), _bits(run_plain(lg, y, perm, ca, cb)))


@pytest.mark.parametrize("c", [pytest.param(c, id=L.iou_id(c)) for c in C.IGN_CASES])
def test_null_map_is_the_plain_entry_point(c, mode):
    """NULL map: dlogits bit-equal to the plain entry point in any mode, S in deterministic mode (default mode: atomics in any order,
    so the exact-regime sums, which have one value in every order, are compared there)"""
    det = mode == "deterministic"
    d = (_cached(("normal", L.iou_id(c), "n2", "zero"), lambda: C.normal_data(c, "n2", "zero")) if det else
         _cached(("exact", L.iou_id(c), "zero"), lambda: C.exact_data(c, "zero")))
    lg, y, perm, ca, cb = (_dev(d[k]) for k in ("logits", "y", "perm", "ca", "cb"))
    assert torch.equal(_bits(run_sums(lg, y, None)), _bits(run_plain(lg, y)))
    assert torch.equal(_bits(run_bwd(lg, y, None, perm, ca, cb)), _bits(run_plain(lg, y, perm, ca, cb)))


@pytest.mark.parametrize("c", [pytest.param(c, id=L.iou_id(c)) for c in C.IGN_CASES])
def test_all_ones_map_costs_one(c, mode):
    """an image ignored everywhere: S = 0, every cost exactly 1.0f, zero gradient"""
    from rsis_amd import ops
    d = _cached(("normal", L.iou_id(c), "hot", "ones"), lambda: C.normal_data(c, "hot", "ones"))
    lg, y, ign, perm, ca, cb = (_dev(d[k]) for k in ("logits", "y", "ignore", "perm", "ca", "cb"))
    S = run_sums(lg, y, ign)
    assert int((_bits(S) != 0).sum()) == 0
    cost = ops.softiou_cost_matrix(S)
    assert torch.equal(cost, torch.ones_like(cost))
    matched = ops.softiou_matched(lg, y, perm, S, ignore=ign)
    assert torch.equal(matched, torch.ones_like(matched))
    assert int((_bits(run_bwd(lg, y, ign, perm, ca, cb)) != 0).sum()) == 0


def test_refusals_write_nothing():
    """with a map: the refusals of the plain entry points, and a map that is not 4-byte aligned"""
    A = _abi()
    Lb, p, st = A.lib(), A.ptr, A.stream()
    lg, y = torch.zeros((2, 3, 16), device="cuda"), torch.ones((2, 4, 16), device="cuda")
    ig = torch.zeros((2 * 16 + 4,), dtype=torch.uint8, device="cuda")
    S = Guarded((3, 4, 5))
    for args in ((p(lg), p(y), p(ig), p(S.t), 0, 3, 4, 16), (p(lg), p(y), p(ig), p(S.t), 2, 0, 4, 16), (p(lg), p(y), p(ig), p(S.t), 2, 3, 0, 16),
                 (p(lg), p(y), p(ig), p(S.t), 2, 129, 4, 16), (p(lg), p(y), p(ig), p(S.t), 2, 3, 129, 16), (p(lg), p(y), p(ig), p(S.t), 2, 3, 4, 12),
                 (None, p(y), p(ig), p(S.t), 2, 3, 4, 16), (p(lg), p(y), p(ig), None, 2, 3, 4, 16), (p(lg), p(y), p(ig) + 1, p(S.t), 2, 3, 4, 16),
                 (p(lg), p(y), None, p(S.t), 2, 3, 4, 12)):
        assert Lb.rsis_softiou_sums_ignore(*args, st) == ERR_ARG, args[4:]
    perm = torch.zeros((2, 5), dtype=torch.int64, device="cuda")
    ca = torch.ones((2, 3), device="cuda")
    dl = Guarded((2, 3, 16))
    for args in ((p(lg), p(y), p(ig), p(perm), 2, p(ca), p(ca), p(dl.t), 2, 3, 4, 16), (p(lg), p(y), p(ig), p(perm), 5, p(ca), p(ca), p(dl.t), 2, 3, 4, 14),
                 (p(lg), p(y), p(ig) + 2, p(perm), 5, p(ca), p(ca), p(dl.t), 2, 3, 4, 16), (p(lg), p(y), p(ig), None, 5, p(ca), p(ca), p(dl.t), 2, 3, 4, 16),
                 (p(lg), p(y), None, p(perm), 2, p(ca), p(ca), p(dl.t), 2, 3, 4, 16)):
        assert Lb.rsis_softiou_bwd_ignore(*args, st) == ERR_ARG, args[4]
    torch.cuda.synchronize()
    S.check("S"), dl.check("dlogits")
    assert S.untouched() and dl.untouched()


# ---------------------------------------------------------------------------------------------------------------------- autograd
def test_autograd_op(mode):
    """ops.softiou_sums / softiou_matched with ignore=: the gradient of sum g * cost against the float64 statement on b3_t10_g20_n4096.
    Bar: K_DLOGITS roundings of the kernel, plus the fp32 coefficients ca = -g / U, cb = g I / U^2 formed from sums each within
    E = M_IOU_IGN * err_host: |d ca| <= |g| 3 E / U^2 + 3 u |ca|, |d cb| <= |g| 7 E / U^2 + 4 u |cb| (I <= U), times p (1 - p) <= 1 / 4."""
    from rsis_amd import ops
    c = [c for c in C.IGN_CASES if L.iou_id(c) == "b3_t10_g20_n4096"][0]
    d = _cached(("normal", L.iou_id(c), "n2", "p30"), lambda: C.normal_data(c, "n2", "p30"))
    B, T = c["B"], c["T"]
    g = np.random.default_rng(5).normal(0, 1, (B, T)).astype(np.float32)
    ref, U, coef = C.matched_grad64(d["logits"], d["y"], d["ignore"], d["perm"], g.astype(np.float64))
    lg = _dev(d["logits"]).requires_grad_()
    y, ign, perm = _dev(d["y"]), _dev(d["ignore"]), _dev(d["perm"])
    S = ops.softiou_sums(lg, y, ignore=ign)
    cost = ops.softiou_matched(lg, y, perm, S, ignore=ign)
    (cost * _dev(g)).sum().backward()
    _zero_bits_under_ignore(lg.grad, ign)
    E = C.M_IOU_IGN * d["err_host"]
    bar = (L.K_DLOGITS * U24 * (np.abs(ref) + coef[:, :, None]) +
           0.25 * (np.abs(g.astype(np.float64)) * 7 * E / (U * U) + 4 * U24 * coef)[:, :, None])
    over = np.abs(lg.grad.double().cpu().numpy() - ref) - bar
    assert over.max() <= 0, "autograd dlogits: %.3e over the bar" % over.max()
    # and the keyword is what routes the call: without it the same op gives the unmasked gradient
    lg2 = _dev(d["logits"]).requires_grad_()
    (ops.softiou_matched(lg2, y, perm, ops.softiou_sums(lg2, y)) * _dev(g)).sum().backward()
    assert not torch.equal(lg2.grad, lg.grad)
