"""fp32 BatchNorm with the ReLU mask kept as bytes (rsis_bn_fwd_mask / rsis_bn_bwd_mask / rsis_bn_bwd_eval_mask, csrc/pointwise.hip): the
forward leaves one byte per float4 group of y (bit k = y[4 i + k] > 0) and the backward reads it instead of y.  Per case:

  1. the mask bytes EQUAL (y > 0) packed by torch from the y the forward returned, and y itself has the bits rsis_bn_fwd writes;
  2. dx, dres, dgamma, dbeta of the mask entry points have the BITS of those of rsis_bn_bwd / rsis_bn_bwd_eval given y;
  3. dx, dres, dgamma, dbeta through ops.batchnorm agree with float64 torch autograd of relu(bn(x) + res) within the bar
     tests/test_gpu_ops.py::test_batchnorm uses (same input distributions): dx 5e-5 + 1e-4 |ref|, dgamma / dbeta 1e-4 + 1e-4 |ref|,
     dres 1e-6; and ops.batchnorm's dx / dres have the bits of the direct call (it runs the mask entry points).

Shapes: the smallest that reach every kernel and its edges (bn_fused_ok and the N / 4 rules of rsis_l_bn_fwd / rsis_l_bn_bwd); eval mode
runs bn_apply_kernel and the two-pass backward at every shape, so a two-pass backward also reads masks at the fused shapes.  7 x 7 maps
(H W % 4 != 0) have no mask: the mask entry points return RSIS_ERR_UNSUPPORTED before launching anything and ops.batchnorm keeps y.

Inputs: the distributions of test_batchnorm, plus one channel with gamma = beta = 0 and a zero residual (y is exactly +0.0 there: mask
bit 0, no gradient) holding one -0.0 residual element, and -- assertion 2 -- a second pass over a copy of y with elements forced to -0.0
and +0.0.  Float32 and float64 must agree on the SIGN of every pre-activation for assertion 3 to mean anything (a flipped ReLU moves
dres by |dy|), so inputs whose float64 pre-activation lies within 1e-3 of zero are pushed away from it and the test asserts that none is
left within 1e-4 (float32 evaluates it to ~1e-6).

Not here: RSIS_BN_FUSED=0 (two-pass kernels at the fused shapes in train mode).  The library reads it once per process, so it cannot be
selected inside this process; the eval-mode cases and the two two-pass shapes run the same kernels.

In the default mode the two-pass kernels add per-block double sums with atomics, in any order.  The terms are floats summed in double:
two orders differ by ~1e-16 relative, which changes the float32 value of a sum with probability ~2^-29, so the bit comparisons hold in
the default mode as well; the case with several blocks per channel is also run in the deterministic mode (one block per channel)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 3           # RSIS_ERR_UNSUPPORTED of csrc/common.h
EPS, MOMENTUM = 1e-5, 0.1
GUARD, FILL = 64, 0xA5

SHAPES = [
    # (B, C, H, W)        forward / train backward kernel
    (2, 64, 8, 8),        # <512,4>, most lanes idle
    (2, 64, 64, 64),      # <512,4>, N / 4 = 2048: the boundary
    (2, 520, 4, 4),       # <256,8> (C > 512)
    (2, 64, 64, 80),      # <1024,8>, N / 4 = 2560
    (2, 3, 16, 16),       # two-pass, C < 64
    (3, 64, 112, 112),    # two-pass, N / 4 > 8192, several blocks per channel
]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pack(y):
    """(y > 0) of every float4 group as one byte, bit k = element k"""
    w = torch.tensor([1, 2, 4, 8], dtype=torch.int32, device=y.device)
    return ((y.reshape(-1, 4) > 0).to(torch.int32) * w).sum(1).to(torch.uint8)


def _ref64(x, r, gamma, beta, rm, rv, train):
    t = F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), training=train, momentum=MOMENTUM, eps=EPS)
    return t + r.double() if r is not None else t


def _inputs(shape, res, train):
    """CPU float32 inputs (x, r, gamma, beta, rm, rv, gy); channel zc has gamma = beta = 0 and a zero residual"""
    B, C, H, W = shape
    rng = np.random.default_rng(1000 * C + H * W + 2 * int(res) + int(train))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    x = f(rng.normal(0.5, 2.0, shape))
    r = f(rng.normal(0, 1, shape)) if res else None
    gamma = f(rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.25, -1.0, 1.0))
    beta = f(rng.normal(0, 0.3, C))
    rm, rv = f(rng.normal(0, 0.1, C)), f(np.abs(rng.normal(0, 0.1, C)) + 0.5)
    gy = f(rng.normal(0, 1, shape))
    zc = C // 2
    gamma[zc], beta[zc] = 0.0, 0.0
    if res:
        r[:, zc] = 0.0
        r[0, zc, 0, 0] = -0.0
    live = torch.ones(C, dtype=torch.bool)
    live[zc] = False
    # keep every pre-activation of the other channels away from the ReLU's kink (see the module docstring)
    near = (_ref64(x, r, gamma, beta, rm, rv, train).abs() < 1e-3) & live.view(1, C, 1, 1)
    if res:
        r[near] += 0.01
    else:
        x[near] += 0.05 * torch.sign(gamma).view(1, C, 1, 1).expand(shape)[near]     # moves the pre-activation by >= 0.05 * 0.5 * rstd
    t = _ref64(x, r, gamma, beta, rm, rv, train)
    assert float(t[:, live].abs().min()) > 1e-4, "test inputs: a pre-activation is still at the ReLU's kink"
    assert bool((t[:, zc] == 0).all())
    return x, r, gamma, beta, rm, rv, gy, zc


class _Bytes(object):
    """n mask bytes as a view into a larger allocation, FILL on both sides and inside"""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]

    def check(self):
        assert bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[-GUARD:] == FILL).all()), "mask: bytes outside the mask were written"


def _forward(entry, x, r, gamma, beta, rm, rv, train, mask=None):
    """rsis_bn_fwd (relu = 1) or rsis_bn_fwd_mask -> (status, y, save_mean, save_rstd, running_mean, running_var)"""
    from rsis_amd._lib import lib, ptr, stream
    B, C, H, W = x.shape
    y = torch.full_like(x, float("nan"))
    stats = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    sm, sr = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    rm, rv = rm.clone(), rv.clone()
    head = (ptr(x), ptr(r), ptr(y)) + ((ptr(mask),) if entry == "rsis_bn_fwd_mask" else ())
    tail = (int(train), stream()) if entry == "rsis_bn_fwd_mask" else (1, int(train), stream())
    st = getattr(lib(), entry)(*head, ptr(stats), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(sm), ptr(sr), B, C, H * W, EPS, MOMENTUM, *tail)
    return st, y, sm, sr, rm, rv


def _backward(entry, dy, x, keep, a, b, gamma, want_dres):
    """one of the four backward entry points -> (status, dx, dres, dgamma, dbeta); keep = y or the mask, (a, b) = saved mean / rstd or
    running mean / var"""
    from rsis_amd._lib import lib, ptr, stream
    B, C, H, W = x.shape
    stats = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    dx = torch.full_like(x, float("nan"))
    dres = torch.full_like(x, float("nan")) if want_dres else None
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    args = [ptr(dy), ptr(x), ptr(keep), ptr(a), ptr(b), ptr(gamma), ptr(stats), ptr(dx), ptr(dres), ptr(dg), ptr(db), B, C, H * W]
    args += [EPS, 1] if "eval" in entry else [1]
    st = getattr(lib(), entry)(*args, stream())
    return st, dx, dres, dg, db


def _same_bits(what, got, want):
    for name, g, w in zip(("dx", "dres", "dgamma", "dbeta"), got, want):
        if w is None:
            assert g is None
            continue
        assert torch.equal(_bits(g), _bits(w)), "%s: %s differs from the y path in %d elements" % (what, name, int((_bits(g) != _bits(w)).sum()))


def _run_case(shape, res, train):
    from rsis_amd import ops
    x, r, gamma, beta, rm, rv, gy, zc = _inputs(shape, res, train)
    xd, gd, bd, rmd, rvd, gyd = (t.cuda() for t in (x, gamma, beta, rm, rv, gy))
    rd = r.cuda() if res else None
    n = x.numel()

    # forward: y as rsis_bn_fwd writes it, the mask beside it
    mask = _Bytes(n // 4)
    st, y, sm, sr, rm1, rv1 = _forward("rsis_bn_fwd_mask", xd, rd, gd, bd, rmd, rvd, train, mask.t)
    assert st == 0
    st, y0, sm0, sr0, rm0, rv0 = _forward("rsis_bn_fwd", xd, rd, gd, bd, rmd, rvd, train)
    assert st == 0
    torch.cuda.synchronize()
    mask.check()
    assert torch.equal(_bits(y), _bits(y0)), "the forward output changed with the mask"
    assert torch.equal(rm1, rm0) and torch.equal(rv1, rv0)
    if train:
        assert torch.equal(sm, sm0) and torch.equal(sr, sr0)
    assert torch.equal(mask.t, _pack(y)), "mask bytes are not (y > 0)"                                    # 1.
    assert bool((y[:, zc] == 0).all()) and bool((mask.t.view(shape[0], shape[1], -1)[:, zc] == 0).all())

    # backward: the mask entry point against the y entry point, bit for bit
    a, b = (sm, sr) if train else (rmd, rvd)
    old, new = ("rsis_bn_bwd", "rsis_bn_bwd_mask") if train else ("rsis_bn_bwd_eval", "rsis_bn_bwd_eval_mask")
    st0, *want = _backward(old, gyd, xd, y, a, b, gd, res)
    st1, *got = _backward(new, gyd, xd, mask.t, a, b, gd, res)
    assert st0 == 0 and st1 == 0
    _same_bits("forward's y", got, want)                                                                  # 2.
    y2 = y.clone()                                           # ... and with -0.0 / +0.0 where the forward had positive values
    pos = torch.nonzero(y2.flatten() > 0).flatten()
    y2.view(-1)[pos[0::7]] = -0.0
    y2.view(-1)[pos[3::7]] = 0.0
    m2 = _pack(y2)
    st0, *want2 = _backward(old, gyd, xd, y2, a, b, gd, res)
    st1, *got2 = _backward(new, gyd, xd, m2, a, b, gd, res)
    assert st0 == 0 and st1 == 0
    _same_bits("y with signed zeros", got2, want2)

    # ops.batchnorm (autograd) against float64, and against the direct call
    x64, g64, b64 = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    r64 = r.double().requires_grad_() if res else None
    t = F.batch_norm(x64, rm.double(), rv.double(), g64, b64, training=train, momentum=MOMENTUM, eps=EPS)
    ref = F.relu(t + r64 if res else t)
    ref.backward(gy.double())
    xa, ga, ba = xd.clone().requires_grad_(), gd.clone().requires_grad_(), bd.clone().requires_grad_()
    ra = rd.clone().requires_grad_() if res else None
    ya = ops.batchnorm(xa, ga, ba, rmd.clone(), rvd.clone(), train, relu=True, res=ra, eps=EPS, momentum=MOMENTUM)
    ya.backward(gyd)
    assert torch.equal(_bits(ya), _bits(y))
    assert torch.equal(_bits(xa.grad), _bits(got[0])), "ops.batchnorm's dx is not the mask entry point's"
    assert_close("fwd", ya, ref, 2e-5, 1e-5)
    assert_close("dx", xa.grad, x64.grad, 5e-5, 1e-4)                                                     # 3.
    assert_close("dgamma", ga.grad, g64.grad, 1e-4, 1e-4)
    assert_close("dbeta", ba.grad, b64.grad, 1e-4, 1e-4)
    if res:
        assert torch.equal(_bits(ra.grad), _bits(got[1]))
        assert_close("dres", ra.grad, r64.grad, 1e-6)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_paths(shape, res, train):
    _run_case(shape, res, train)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_mask_two_pass_one_block_per_channel(train):
    """the several-blocks case again in the deterministic mode: one block per channel, no atomics between blocks"""
    from rsis_amd import ops
    prev = ops.set_deterministic(True)
    try:
        _run_case(SHAPES[-1], True, train)
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
def test_no_mask_on_7x7_maps(res, train):
    """H W % 4 != 0: the mask entry points refuse before launching anything (outputs untouched); ops.batchnorm keeps y and still agrees
    with float64"""
    from rsis_amd import ops
    shape = (2, 64, 7, 7)
    x, r, gamma, beta, rm, rv, gy, zc = _inputs(shape, res, train)
    xd, gd, bd, rmd, rvd, gyd = (t.cuda() for t in (x, gamma, beta, rm, rv, gy))
    rd = r.cuda() if res else None
    mask = _Bytes((x.numel() + 3) // 4)
    st, y, sm, sr, rm1, rv1 = _forward("rsis_bn_fwd_mask", xd, rd, gd, bd, rmd, rvd, train, mask.t)
    torch.cuda.synchronize()
    assert st == ERR_UNSUPPORTED
    assert bool(torch.isnan(y).all()) and bool((mask.buf == FILL).all()) and torch.equal(rm1, rmd) and torch.equal(rv1, rvd)
    for entry in ("rsis_bn_bwd_mask", "rsis_bn_bwd_eval_mask"):
        st, dx, dres, dg, db = _backward(entry, gyd, xd, mask.t, rmd, rvd, gd, res)
        torch.cuda.synchronize()
        assert st == ERR_UNSUPPORTED and bool(torch.isnan(dx).all())

    x64, g64, b64 = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    r64 = r.double().requires_grad_() if res else None
    t = F.batch_norm(x64, rm.double(), rv.double(), g64, b64, training=train, momentum=MOMENTUM, eps=EPS)
    ref = F.relu(t + r64 if res else t)
    ref.backward(gy.double())
    xa, ga, ba = xd.clone().requires_grad_(), gd.clone().requires_grad_(), bd.clone().requires_grad_()
    ra = rd.clone().requires_grad_() if res else None
    ya = ops.batchnorm(xa, ga, ba, rmd.clone(), rvd.clone(), train, relu=True, res=ra, eps=EPS, momentum=MOMENTUM)
    ya.backward(gyd)
    assert_close("fwd", ya, ref, 2e-5, 1e-5)
    assert_close("dx", xa.grad, x64.grad, 5e-5, 1e-4)
    assert_close("dgamma", ga.grad, g64.grad, 1e-4, 1e-4)
    assert_close("dbeta", ba.grad, b64.grad, 1e-4, 1e-4)
    if res:
        assert_close("dres", ra.grad, r64.grad, 1e-6)


def test_inference_writes_no_mask():
    """under no_grad nothing is back-propagated: ops.batchnorm runs rsis_bn_fwd and allocates no mask (same output bits), also with
    parameters that require a gradient"""
    from rsis_amd import ops
    x, r, gamma, beta, rm, rv, gy, zc = _inputs((2, 64, 8, 8), True, False)
    xd, rd, gd, bd, rmd, rvd = (t.cuda() for t in (x, r, gamma, beta, rm, rv))
    gd.requires_grad_()
    bd.requires_grad_()
    st, y0, *_ = _forward("rsis_bn_fwd", xd, rd, gd, bd, rmd, rvd, False)
    assert st == 0
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        y = ops.batchnorm(xd, gd, bd, rmd, rvd, False, relu=True, res=rd, eps=EPS, momentum=MOMENTUM)
    assert torch.cuda.memory_allocated() - before == y.numel() * 4
    assert torch.equal(_bits(y), _bits(y0))
