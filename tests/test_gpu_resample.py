"""The fp32 resize and pooling kernels of rsis_amd/csrc/pointwise.hip on every launch path, through the C entry points: bilinear
align-corners upsample forward / backward (/ with the global pool's gradient folded in), global max-pool, MaxPool2d(3, 2, 1).  Cases,
restated launch rules and float64 references: resample_cases.py (checked on the host by test_resample_host.py).

Every output is a view into a larger allocation with guard elements of a byte pattern on both sides, prefilled with NaN (floats) or an
impossible value (arg-max indices); afterwards the guards must be untouched and no prefill left.  Every launch runs in the default and in
the deterministic mode of the library and must give the same bits in both.

Bars (u = 2^-24; derivations in resample_cases.up_fwd_refs / up_bwd_refs).  The worst error / bar of each of the four upsample
comparisons goes to the RSIS_TEST_MARGINS survey of helpers.assert_close under the names up_fwd/model, up_fwd/ref, up_bwd/model,
up_bwd/ref; the figures are recorded, they are not where the bars come from.
  forward  vs model A_h x A_w^T:      8u (|A_h| |x| |A_w|^T); the identity resize bit for bit
  forward  vs F.interpolate, float64:  the above + delta_h max|x[h+1] - x[h]| + delta_w max|x[w+1] - x[w]|, delta = 2u (in - 1)
  backward vs model A_h^T dy A_w:      (2 (k_h + k_w) + 2) u (|A_h|^T |dy| |A_w| + |pool_g| at the arg-max)
  backward vs float64 autograd:        the above + the same delta over the outputs that can touch an input
  pools: values, arg-max indices and (integer dy) gradients equal to F.max_pool2d on float64 copies, exactly"""
import contextlib

import numpy as np
import pytest
import torch

import resample_cases as R
from helpers import assert_close

pytestmark = pytest.mark.gpu

G = 64                      # guard elements on each side (of the tensor's dtype: the view stays 16-byte aligned)
PATTERN = 0xA5
PREFILL = {torch.float32: float("nan"), torch.int32: -1, torch.uint8: 0xEE}


class Guarded(object):
    def __init__(self, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape))
        self.isz = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * G) * self.isz,), PATTERN, dtype=torch.uint8, device="cuda")
        self.lo, self.hi = G * self.isz, (G + n) * self.isz
        self.t = self.raw[self.lo:self.hi].view(dtype).view(*shape)
        self.dtype = dtype
        if init is None:
            self.t.fill_(PREFILL[dtype])
        else:
            self.t.copy_(torch.as_tensor(init))

    def check(self, what):
        assert bool((self.raw[:self.lo] == PATTERN).all()), "%s: the guard zone in FRONT of the output was written" % what
        assert bool((self.raw[self.hi:] == PATTERN).all()), "%s: the guard zone BEHIND the output was written" % what
        if self.dtype == torch.float32:
            assert not bool(torch.isnan(self.t).any()), "%s: %d elements were never written (or are NaN)" % (what, int(torch.isnan(self.t).sum()))
        else:
            assert not bool((self.t == PREFILL[self.dtype]).any()), "%s: elements were never written" % what
        return self.t


@contextlib.contextmanager
def deterministic(on):
    from rsis_amd._lib import lib
    prev = lib().rsis_set_deterministic(1 if on else 0)
    try:
        yield
    finally:
        lib().rsis_set_deterministic(prev)


def both_modes(run, what):
    """run() in the default and in the deterministic mode: the same bits; returns the default mode's result (tensors on the host)"""
    outs = []
    for det in (0, 1):
        with deterministic(det):
            outs.append([o.cpu() for o in run()])
    for a, b in zip(*outs):
        assert torch.equal(a, b), "%s: the deterministic mode gives other bits" % what
    return outs[0]


def within_bar(what, got, want, bar):
    """|got - want| <= bar element-wise (float64 arrays); where the bar is 0 the values must be equal.  Compared as err / bar against 1, so
    that the margin survey of assert_close records the worst err / bar."""
    got = got.double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isfinite(got), ratio, np.nan)
    print("%s: worst err / bar %.3f (max err %.3e)" % (what, float(np.nanmax(ratio)) if ratio.size else 0.0, float(np.nanmax(err)) if err.size else 0.0))
    assert_close(what, ratio, np.zeros_like(ratio), 1.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- upsample forward
@pytest.mark.parametrize("c", R.UP_FWD, ids=R.case_id)
def test_upsample_fwd(c):
    from rsis_amd._lib import check, lib, ptr, stream
    r = R.up_fwd_refs(c)
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    x = dev(r["x"])

    def run():
        y = Guarded((BC, Ho, Wo))
        check(lib().rsis_upsample_bilinear_ac_fwd(ptr(x), ptr(y.t), BC, Hi, Wi, Ho, Wo, stream()), "rsis_upsample_bilinear_ac_fwd")
        return [y.check("y (%s)" % c["path"])]

    got, = both_modes(run, c["path"])
    if c.get("identity"):
        assert torch.equal(got, torch.from_numpy(r["x"])), "the identity resize changed bits"
    within_bar("up_fwd/model", got, r["model"], r["bar_model"])
    within_bar("up_fwd/ref", got, r["ref"], r["bar_ref"])


# ---------------------------------------------------------------- upsample backward, plain and with the pool gradient folded in
@pytest.mark.parametrize("c", R.UP_BWD, ids=R.case_id)
def test_upsample_bwd(c):
    from rsis_amd._lib import check, lib, ptr, stream
    r = R.up_bwd_refs(c)
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    dy, pool_g, arg = dev(r["dy"]), dev(r["pool_g"]), dev(r["pool_arg"])
    L = lib()

    def run():
        dx = Guarded((BC, Hi, Wi))
        check(L.rsis_upsample_bilinear_ac_bwd(ptr(dy), ptr(dx.t), BC, Hi, Wi, Ho, Wo, stream()), "rsis_upsample_bilinear_ac_bwd")
        plain = dx.check("dx (%s)" % c["path"]).clone()
        check(L.rsis_global_maxpool_bwd_add(ptr(pool_g), ptr(arg), ptr(dx.t), BC, Hi * Wi, stream()), "rsis_global_maxpool_bwd_add")
        two = dx.check("dx after the pool add")
        fused = Guarded((BC, Hi, Wi))
        check(L.rsis_upsample_maxpool_bwd(ptr(dy), ptr(pool_g), ptr(arg), ptr(fused.t), BC, Hi, Wi, Ho, Wo, stream()), "rsis_upsample_maxpool_bwd")
        return [plain, two, fused.check("dx of the fused launch (%s)" % c["path"])]

    plain, two, fused = both_modes(run, c["path"])
    within_bar("up_bwd/model", plain, r["model"], r["bar_model"])
    within_bar("up_bwd/ref", plain, r["ref"], r["bar_ref"])
    within_bar("up_bwd/model", fused, r["model_pool"], r["bar_model_pool"])
    assert torch.equal(fused, two), "rsis_upsample_maxpool_bwd != rsis_upsample_bilinear_ac_bwd followed by rsis_global_maxpool_bwd_add"


def test_upsample_through_ops_autograd():
    from rsis_amd import ops
    c = next(c for c in R.UP_FWD if c["path"] == "lds32x64" and c["Ho"] % 32)
    r = R.up_fwd_refs(c)
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    x = dev(r["x"]).view(1, BC, Hi, Wi).requires_grad_()
    y = ops.upsample_bilinear_ac(x, (Ho, Wo))
    within_bar("up_fwd/model", y.detach().cpu()[0], r["model"], r["bar_model"])
    dy = R._normal(77, (BC, Ho, Wo))
    y.backward(dev(dy).view(1, BC, Ho, Wo))
    Ah, Aw = R.resize_matrices(Hi, Ho, Wi, Wo)
    k = (2 * (int((Ah != 0).sum(0).max()) + int((Aw != 0).sum(0).max())) + 2) * R.U
    within_bar("up_bwd/model", x.grad.cpu()[0], Ah.T @ dy.astype(np.float64) @ Aw, k * (np.abs(Ah).T @ np.abs(dy.astype(np.float64)) @ np.abs(Aw)))


# ---------------------------------------------------------------- global max-pool
@pytest.mark.parametrize("c", R.GMAX_FWD, ids=R.case_id)
def test_global_maxpool_fwd_bwd(c):
    from rsis_amd._lib import check, lib, ptr, stream
    BC, HW = c["BC"], c["HW"]
    xh = R.gmax_data(c)
    v_ref, a_ref = R.gmax_ref(xh)
    x = dev(xh)
    dyh = np.random.default_rng(R.case_seed(c) + 1).integers(-3, 4, BC).astype(np.float32)
    dy = dev(dyh)
    L = lib()

    def run():
        y, arg, dx = Guarded((BC,)), Guarded((BC,), torch.int32), Guarded((BC, HW))
        check(L.rsis_global_maxpool_fwd(ptr(x), ptr(y.t), ptr(arg.t), BC, HW, stream()), "rsis_global_maxpool_fwd")
        check(L.rsis_global_maxpool_bwd(ptr(dy), ptr(arg.check("arg")), ptr(dx.t), BC, HW, stream()), "rsis_global_maxpool_bwd")
        return [y.check("y"), arg.t, dx.check("dx")]

    y, arg, dx = both_modes(run, c["path"])
    assert np.array_equal(y.double().numpy(), v_ref), "pooled values differ from F.max_pool2d"
    assert np.array_equal(arg.numpy().astype(np.int64), a_ref), "arg-max: got %s want %s (the FIRST maximum in row-major order)" % (arg.numpy(), a_ref)
    want = np.zeros((BC, HW))
    want[np.arange(BC), a_ref] = dyh
    assert np.array_equal(dx.double().numpy(), want), "gradient is not dy at the arg-max and 0 elsewhere"


def test_global_maxpool_bwd_second_trip():
    from rsis_amd._lib import check, lib, ptr, stream
    BC, HW = R.GMAX_BWD_BIG["BC"], R.GMAX_BWD_BIG["HW"]
    rs = np.random.default_rng(31)
    argh = rs.integers(0, HW, BC).astype(np.int32)
    argh[:4] = (0, HW - 1, 0, HW - 1)
    argh[-1] = HW - 1
    dyh = rs.normal(0, 1, BC).astype(np.float32)
    arg, dy = dev(argh), dev(dyh)

    def run():
        dx = Guarded((BC, HW))
        check(lib().rsis_global_maxpool_bwd(ptr(dy), ptr(arg), ptr(dx.t), BC, HW, stream()), "rsis_global_maxpool_bwd")
        return [dx.check("dx")]

    dx, = both_modes(run, "global_maxpool_bwd")
    want = np.zeros((BC, HW), np.float32)
    want[np.arange(BC), argh] = dyh
    assert np.array_equal(dx.numpy(), want)


def test_global_maxpool_bwd_add_into_a_filled_gradient():
    from rsis_amd._lib import check, lib, ptr, stream
    BC, HW = R.GMAX_BWD_ADD["BC"], R.GMAX_BWD_ADD["HW"]
    rs = np.random.default_rng(32)
    argh = rs.integers(0, HW, BC).astype(np.int32)
    argh[0], argh[-1] = 0, HW - 1
    dyh, pre = rs.normal(0, 1, BC).astype(np.float32), rs.normal(0, 1, (BC, HW)).astype(np.float32)
    arg, dy = dev(argh), dev(dyh)

    def run():
        dx = Guarded((BC, HW), init=pre)
        check(lib().rsis_global_maxpool_bwd_add(ptr(dy), ptr(arg), ptr(dx.t), BC, HW, stream()), "rsis_global_maxpool_bwd_add")
        return [dx.check("dx")]

    dx, = both_modes(run, "global_maxpool_bwd_add")
    want = pre.copy()
    want[np.arange(BC), argh] += dyh                    # one fp32 addition: the same bits
    assert np.array_equal(dx.numpy(), want)


def test_global_maxpool_through_ops_autograd():
    from rsis_amd import ops
    c = next(c for c in R.GMAX_FWD if c["kind"] == "ties" and c["HW"] == 16384)
    xh = R.gmax_data(c)
    v_ref, a_ref = R.gmax_ref(xh)
    x = dev(xh).view(2, c["BC"] // 2, 128, 128).requires_grad_()
    y = ops.global_maxpool(x)
    assert np.array_equal(y.detach().cpu().double().numpy().reshape(-1), v_ref)
    gy = np.arange(1, c["BC"] + 1, dtype=np.float32)
    y.backward(dev(gy).view_as(y))
    want = np.zeros((c["BC"], c["HW"]), np.float32)
    want[np.arange(c["BC"]), a_ref] = gy
    assert np.array_equal(x.grad.cpu().numpy().reshape(c["BC"], -1), want)


# ---------------------------------------------------------------- MaxPool2d(3, stride 2, pad 1)
# (the two cases that reach a second trip run once, on the data with ties)
@pytest.mark.parametrize("c,ties", [(c, t) for c in R.MAXPOOL for t in (False, True) if t or c["items"] <= R.TWO20],
                         ids=lambda v: R.case_id(v) if isinstance(v, dict) else ("ties" if v else "cont"))
def test_maxpool3x3s2_fwd_bwd(c, ties):
    from rsis_amd._lib import check, lib, ptr, stream
    BC, H, W = c["BC"], c["H"], c["W"]
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    xh, dyh, preh = R.maxpool_data(c, ties)
    v_ref, i_ref, g_ref = R.maxpool_ref(xh, dyh)
    x, dy = dev(xh), dev(dyh)
    L = lib()

    def run():
        y, arg = Guarded((BC, Ho, Wo)), Guarded((BC, Ho, Wo), torch.uint8)
        check(L.rsis_maxpool3x3s2_fwd(ptr(x), ptr(y.t), ptr(arg.t), BC, H, W, Ho, Wo, stream()), "rsis_maxpool3x3s2_fwd")
        outs = [y.check("y"), arg.check("arg")]
        for accumulate in (0, 1):
            dx = Guarded((BC, H, W), init=preh if accumulate else None)
            check(L.rsis_maxpool3x3s2_bwd(ptr(dy), ptr(arg.t), ptr(dx.t), BC, H, W, Ho, Wo, accumulate, stream()), "rsis_maxpool3x3s2_bwd")
            outs.append(dx.check("dx (%s, accumulate %d)" % (c["path"], accumulate)))
        return outs

    y, arg, dx0, dx1 = both_modes(run, c["path"])
    assert np.array_equal(y.double().numpy(), v_ref), "pooled values differ from F.max_pool2d"
    a = arg.numpy().astype(np.int64)
    ho, wo = np.arange(Ho)[None, :, None], np.arange(Wo)[None, None, :]
    assert a.max() <= 8 and np.array_equal((2 * ho - 1 + a // 3) * W + (2 * wo - 1 + a % 3), i_ref), "arg-max byte: not the FIRST maximum of the window"
    assert np.array_equal(dx0.double().numpy(), g_ref), "gradient differs from the scatter of dy at F.max_pool2d's indices"
    assert np.array_equal(dx1.double().numpy(), g_ref + preh), "accumulate: gradient + prefill differs"


def test_maxpool3x3s2_through_ops_autograd():
    from rsis_amd import ops
    c = next(c for c in R.MAXPOOL if (c["H"], c["W"]) == (9, 11))
    xh, dyh, _ = R.maxpool_data(c, True)
    v_ref, _, g_ref = R.maxpool_ref(xh, dyh)
    x = dev(xh).view(3, c["BC"] // 3, 9, 11).requires_grad_()
    y = ops.maxpool3x3s2(x)
    assert np.array_equal(y.detach().cpu().double().numpy().reshape(v_ref.shape), v_ref)
    y.backward(dev(dyh).view_as(y))
    assert np.array_equal(x.grad.cpu().double().numpy().reshape(g_ref.shape), g_ref)
