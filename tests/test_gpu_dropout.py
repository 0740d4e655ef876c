"""`-dropout`, `-dropout_cls`, `-dropout_stop` on the one-node sequence decoder (rsis_amd/decoder_seq.py, rsis_amd/dropout.py,
csrc/dropout.hip and the scaled upsample / pool-backward kernels of pointwise.hip / blk_dec.hip).

  generator   rsis_dropout_scales against the numpy restatement of its rule (rsis_amd.dropout.scales_numpy), bit for bit
  kernels     every scaled entry point on the launch paths of tests/resample_cases.py: with scales in {0, 2} EQUAL to scale x the unscaled
              entry point's output; with p = 0.3 within the unscaled kernel's own bar (test_gpu_resample.py, test_gpu_blk_dec.py) times the
              scale; with a NULL scale the unscaled output's bits
  heads       the masked class / stop heads (decoder_seq._heads_fwd_masked / _heads_bwd_masked) in both families against float64, within
              the a priori bounds of heads_wide_cases.py evaluated on the masked features; the mask product and the sum of the two
              masked gradients add gamma(3) of their terms
  decoder     both layouts: the recorded scales replayed into the float64 oracle decoder.  fp32: outputs within 1e-4, gradients within
              1e-4 max(1, max |ref|).  blk bf16: the distances test_gpu_blk_dec.py allows between blk and fp32 storage (outputs 2 % of the
              largest, gradients 6 % relative L2 and 1.5 x the fp32-storage path's own distance from float64 + 1 %), each run against the
              oracle pooled at the pixels that run pooled (_check_blk says why)
  invariance  all rates 0: no state, no scale buffer, torch's generators untouched, the same bits before and after dropout was used
  graph       train.py --graph with all three rates: captured, replayed, fresh masks per replay"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dropout_cases as C
import heads_wide_cases as W
import loss_path_cases as LP
import resample_cases as R
from helpers import assert_close, mk_args
from test_gpu_blk import HALF_ULP, _bf16, from_blk, to_blk
from test_gpu_resample import Guarded, both_modes, dev, within_bar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
U = R.U
KEEP3 = np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))


def _abi():
    from rsis_amd import _lib
    return _lib


def _state(rank=0):
    from rsis_amd import dropout as D
    return D.new_state(torch.device("cuda"), seed=C.SEED, rank=rank)


def _plane_scales(seed, n, keep):
    """n factors in {0, keep}, both present"""
    s = np.where(np.random.default_rng(seed).random(n) < 0.5, 0.0, keep).astype(np.float32)
    s[0], s[-1] = (keep, 0.0) if n > 1 else (keep, keep)
    return s


def _bits(t):
    return t.contiguous().view(torch.int32)


# ======================================================================================================================
# generator
# ======================================================================================================================
@pytest.mark.parametrize("n", [C.n_elems(), 1001, 300001], ids=["decoder", "tail_of_a_block", "grid_stride"])
def test_scales_equal_the_numpy_rule_and_the_counter_advances(n):
    from rsis_amd import dropout as D
    A = _abi()
    st = _state()
    words = C.state0()
    for call, rates in enumerate([(0.5, 0.3, 0.0), (0.3, 0.5, 0.5)]):
        out = [Guarded((n,)) for _ in range(3)]
        A.check(A.lib().rsis_dropout_scales(A.ptr(st), A.ptr(out[0].t), A.ptr(out[1].t), A.ptr(out[2].t), n, *rates, A.stream()), "rsis_dropout_scales")
        torch.cuda.synchronize()
        for a, (g, p) in enumerate(zip(out, rates)):
            got = g.check("array %d" % a).cpu().numpy()
            want = D.scales_numpy(words, a, n, p)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "call %d, array %d: %d elements differ" % (call, a, int((got != want).sum()))
            if p == 0.0:
                assert np.array_equal(got, np.ones(n, np.float32))
        if call == 1:
            assert not np.array_equal(got, first), "the second call repeated the first call's masks"
        first = D.scales_numpy(words, 2, n, 0.5)
        words = D.advance(words)
        assert D.state_words(st) == words and st[4:].cpu().tolist() == [0, 0, 0, 0], "state after call %d: %s" % (call, st.cpu().tolist())


def test_ranks_draw_different_masks_on_the_device():
    from rsis_amd import dropout as D
    a, b = D.draw(_state(0), 1024, 0.5, 0.5, 0.5), D.draw(_state(1), 1024, 0.5, 0.5, 0.5)
    assert all(not torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("rates", [(1.0, 0.0, 0.0), (0.0, -0.1, 0.0), (0.0, 0.0, 1.5), (float("nan"), 0.0, 0.0)], ids=["p1", "negative", "above1", "nan"])
def test_scales_refuse_rates_outside_0_1(rates):
    from rsis_amd import dropout as D
    A = _abi()
    st = _state()
    out = [Guarded((64,)) for _ in range(3)]
    rc = A.lib().rsis_dropout_scales(A.ptr(st), A.ptr(out[0].t), A.ptr(out[1].t), A.ptr(out[2].t), 64, *rates, A.stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG
    assert D.state_words(st) == C.state0() and all(bool(torch.isnan(g.t).all()) for g in out), "a refused call wrote something"


# ======================================================================================================================
# fp32 kernels, per launch path
# ======================================================================================================================
@pytest.mark.parametrize("c", R.UP_FWD, ids=R.case_id)
def test_scaled_upsample_fwd(c):
    A = _abi()
    L = A.lib()
    r = R.up_fwd_refs(c)
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    x = dev(r["x"])
    s2h, s3h = _plane_scales(R.case_seed(c), BC, 2.0), _plane_scales(R.case_seed(c) + 1, BC, KEEP3)
    s2, s3 = dev(s2h), dev(s3h)

    def run():
        outs = []
        for sc in (None, s2, s3, "unscaled"):
            y = Guarded((BC, Ho, Wo))
            if isinstance(sc, str):
                A.check(L.rsis_upsample_bilinear_ac_fwd(A.ptr(x), A.ptr(y.t), BC, Hi, Wi, Ho, Wo, A.stream()), "rsis_upsample_bilinear_ac_fwd")
            else:
                A.check(L.rsis_upsample_bilinear_ac_scaled_fwd(A.ptr(x), A.ptr(sc), A.ptr(y.t), BC, Hi, Wi, Ho, Wo, A.stream()), "scaled fwd")
            outs.append(y.check("y (%s)" % c["path"]))
        return outs

    null, two, p3, plain = both_modes(run, c["path"])
    assert torch.equal(_bits(null), _bits(plain)), "a NULL scale does not give the unscaled entry point's bits"
    assert torch.equal(two, plain * torch.from_numpy(s2h)[:, None, None]), "scale in {0, 2}: not scale x the unscaled output"
    assert bool((two[s2h == 0] == 0).all())
    s64 = s3h.astype(np.float64)[:, None, None]
    within_bar("scaled up_fwd/ref", p3, s64 * r["ref"], s64 * r["bar_ref"])


@pytest.mark.parametrize("c", R.UP_BWD, ids=R.case_id)
def test_scaled_upsample_maxpool_bwd(c):
    A = _abi()
    L = A.lib()
    r = R.up_bwd_refs(c)
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    dy, pool_g, arg = dev(r["dy"]), dev(r["pool_g"]), dev(r["pool_arg"])
    s2h, s3h = _plane_scales(R.case_seed(c), BC, 2.0), _plane_scales(R.case_seed(c) + 1, BC, KEEP3)
    s2, s3 = dev(s2h), dev(s3h)

    def run():
        outs = []
        for sc in (None, s2, s3, "unscaled"):
            dx = Guarded((BC, Hi, Wi))
            if isinstance(sc, str):
                A.check(L.rsis_upsample_maxpool_bwd(A.ptr(dy), A.ptr(pool_g), A.ptr(arg), A.ptr(dx.t), BC, Hi, Wi, Ho, Wo, A.stream()), "unscaled bwd")
            else:
                A.check(L.rsis_upsample_maxpool_scaled_bwd(A.ptr(dy), A.ptr(pool_g), A.ptr(arg), A.ptr(sc), A.ptr(dx.t), BC, Hi, Wi, Ho, Wo, A.stream()),
                        "scaled bwd")
            outs.append(dx.check("dx (%s)" % c["path"]))
        return outs

    null, two, p3, plain = both_modes(run, c["path"])
    assert torch.equal(_bits(null), _bits(plain)), "a NULL scale does not give the unscaled entry point's bits"
    assert torch.equal(two, plain * torch.from_numpy(s2h)[:, None, None]), "scale in {0, 2}: not scale x the unscaled output"
    assert bool((two[s2h == 0] == 0).all()), "a plane with scale 0 received a gradient"
    s64 = s3h.astype(np.float64)[:, None, None]
    within_bar("scaled up_bwd/model", p3, s64 * r["model_pool"], s64 * r["bar_model_pool"])


def test_scaled_global_maxpool_bwd_add_and_scale_planes():
    A = _abi()
    L = A.lib()
    BC, HW = R.GMAX_BWD_ADD["BC"], R.GMAX_BWD_ADD["HW"]
    rs = np.random.default_rng(33)
    argh = rs.integers(0, HW, BC).astype(np.int32)
    argh[0], argh[-1] = 0, HW - 1
    dyh, pre = rs.normal(0, 1, BC).astype(np.float32), rs.normal(0, 1, (BC, HW)).astype(np.float32)
    arg, dy = dev(argh), dev(dyh)
    s2h, s3h = _plane_scales(5, BC, 2.0), _plane_scales(6, BC, KEEP3)
    rows = np.arange(BC)

    def add(sc, init):
        dx = Guarded((BC, HW), init=init)
        if isinstance(sc, str):
            A.check(L.rsis_global_maxpool_bwd_add(A.ptr(dy), A.ptr(arg), A.ptr(dx.t), BC, HW, A.stream()), "rsis_global_maxpool_bwd_add")
        else:
            A.check(L.rsis_global_maxpool_scaled_bwd_add(A.ptr(dy), A.ptr(arg), A.ptr(sc), A.ptr(dx.t), BC, HW, A.stream()), "scaled add")
        return dx.check("dx")

    zero = np.zeros_like(pre)
    null, plain, two, plain0, two0, p3 = both_modes(lambda: [add(None, pre), add("unscaled", pre), add(dev(s2h), pre), add("unscaled", zero),
                                                            add(dev(s2h), zero), add(dev(s3h), pre)], "global_maxpool_scaled_bwd_add")
    assert torch.equal(_bits(null), _bits(plain))
    assert torch.equal(two0, plain0 * torch.from_numpy(s2h)[:, None]), "scale in {0, 2} into a zero gradient: not scale x the unscaled output"
    want = pre.copy()
    want[rows, argh] += s2h * dyh                       # an exact product and one fp32 addition: the same bits
    assert np.array_equal(two.numpy(), want)
    # p = 0.3: the product and the sum round once each (or once together, contracted): 2u of the two terms
    ref = pre.astype(np.float64)
    ref[rows, argh] += s3h.astype(np.float64) * dyh
    bar = np.zeros_like(ref)
    bar[rows, argh] = 2 * U * (np.abs(pre[rows, argh]) + np.abs(s3h.astype(np.float64) * dyh))
    within_bar("scaled gmax_bwd_add", p3, ref, bar)
    # the scaled copy (the equal-size resize, either direction): one fp32 product per element, also in place and through the scaled forward
    x = dev(pre)
    for sh in (s2h, s3h):
        y, y2 = Guarded((BC, HW)), Guarded((BC, 8, 8))
        A.check(L.rsis_scale_planes(A.ptr(x), A.ptr(dev(sh)), A.ptr(y.t), BC, HW, A.stream()), "rsis_scale_planes")
        A.check(L.rsis_upsample_bilinear_ac_scaled_fwd(A.ptr(x), A.ptr(dev(sh)), A.ptr(y2.t), BC, 8, 8, 8, 8, A.stream()), "scaled fwd, equal sizes")
        want = pre * sh[:, None]
        assert np.array_equal(y.check("y").cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(y2.check("y2").cpu().numpy().reshape(BC, HW).view(np.uint32), want.view(np.uint32))
    z = Guarded((BC, HW), init=pre)
    A.check(L.rsis_scale_planes(A.ptr(z.t), A.ptr(dev(s3h)), A.ptr(z.t), BC, HW, A.stream()), "rsis_scale_planes in place")
    assert np.array_equal(z.check("z").cpu().numpy().view(np.uint32), (pre * s3h[:, None]).view(np.uint32))


# ======================================================================================================================
# blk kernels
# ======================================================================================================================
def _null_scaled(job):
    """the job of the scaled entry points with a NULL scale, from an unscaled job"""
    A = _abi()
    j = A.BlkResizeScaledJob()
    for k, _t in A.BlkResizeJob._fields_:
        setattr(j, k, getattr(job[0], k))
    return j, job[1]


BLK_SHAPES = [(2, 16, 7, 7, 14, 14), (3, 24, 5, 7, 9, 13), (2, 8, 1, 1, 3, 3), (2, 8, 6, 8, 6, 8), (2, 8, 4, 4, 48, 48), (2, 8, 37, 50, 74, 100)]


@pytest.mark.parametrize("shape", BLK_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_scaled_blk_upsample_forward_and_transpose(shape):
    """(7 -> 14, odd sizes, a 1 x 1 input, equal sizes, a 12-fold upsample whose transpose takes the plain candidate scan, the last level of the
    odd pyramid with several blocks)"""
    from rsis_amd import ops
    F = torch.nn.functional
    B, Cc, Hi, Wi, Ho, Wo = shape
    torch.manual_seed(Hi + Wo)
    x = _bf16(torch.randn(B, Cc, Hi, Wi, device="cuda"))
    dy = _bf16(torch.randn(B, Cc, Ho, Wo, device="cuda"))
    dpool = torch.randn(B, Cc, device="cuda")
    arg = torch.randint(0, Hi * Wi, (B, Cc), device="cuda", dtype=torch.int32)
    s2 = dev(_plane_scales(Hi, B * Cc, 2.0)).view(B, Cc)
    s3 = dev(_plane_scales(Wo, B * Cc, KEEP3)).view(B, Cc)
    xb, dyb = to_blk(x), to_blk(dy)

    def fwd(sc, scaled=True):
        y = torch.empty((B, Cc // 8, Ho, Wo, 8), dtype=torch.bfloat16, device="cuda")
        job = ops.blk_resize_job(xb, y, scale=sc)
        ops.blk_upsample_fwd_batch([_null_scaled(job) if scaled and sc is None else job])
        return y

    def bwd(sc, scaled=True):
        dx = torch.empty((B, Cc // 8, Hi, Wi, 8), dtype=torch.bfloat16, device="cuda")
        job = ops.blk_resize_job(dyb, dx, dpool, arg, backward=True, scale=sc)
        ops.blk_upsample_bwd_batch([_null_scaled(job) if scaled and sc is None else job])
        return dx

    y0, d0 = fwd(None, scaled=False), bwd(None, scaled=False)
    assert torch.equal(_bits(fwd(None)), _bits(y0)), "forward: a NULL scale does not give the unscaled job's bits"
    assert torch.equal(_bits(bwd(None)), _bits(d0)), "transpose: a NULL scale does not give the unscaled job's bits"
    # {0, 2}: doubling commutes with the one rounding to bf16
    f2, b2 = from_blk(fwd(s2)), from_blk(bwd(s2))
    print("scale in {0, 2}: %d forward and %d transpose elements differ from scale x unscaled"
          % (int((f2 != from_blk(y0) * s2.view(B, Cc, 1, 1)).sum()), int((b2 != from_blk(d0) * s2.view(B, Cc, 1, 1)).sum())))
    assert torch.equal(f2, from_blk(y0) * s2.view(B, Cc, 1, 1)), "forward, scale in {0, 2}"
    assert torch.equal(b2, from_blk(d0) * s2.view(B, Cc, 1, 1)), "transpose, scale in {0, 2}"
    # p = 0.3 against float64 on the bf16-valued inputs: the bars of test_blk_upsample_forward_and_transpose_with_pooled_gradient
    xd = x.double().requires_grad_()
    ref = F.interpolate(xd, size=(Ho, Wo), mode="bilinear", align_corners=True)
    ref.backward(dy.double())
    sd = s3.double().view(B, Cc, 1, 1)
    want = ref.detach() * sd
    assert_close("scaled fwd", from_blk(fwd(s3)), want, 2e-5 * float(want.abs().max()), HALF_ULP)
    dref = xd.grad.clone().view(B, Cc, -1)
    dref.scatter_add_(2, arg.long().unsqueeze(-1), dpool.double().unsqueeze(-1))
    dwant = dref.view(B, Cc, Hi, Wi) * sd
    assert_close("scaled bwd + pooled gradient", from_blk(bwd(s3)), dwant, 2e-5 * float(dwant.abs().max()), HALF_ULP)


# ======================================================================================================================
# heads
# ======================================================================================================================
def _drop_of(n, rates, T, B, hs):
    """a decoder_seq._Drop from one generator launch at the tests' state, and the host copies of its three arrays"""
    from rsis_amd import decoder_seq, dropout as D
    d = decoder_seq._Drop()
    d.S2, d.MC, d.MS = D.draw(_state(), n, *rates)
    d.s2 = decoder_seq._per_level(d.S2, hs, T, B)
    d.SIDEC, d.SIDES = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    return d, [D.scales_numpy(C.state0(), a, n, p) for a, p in zip((0, 1, 2), rates)]


@pytest.mark.parametrize("ncls,rates", [(21, (0.5, 0.5, 0.5)), (21, (0.3, 0.3, 0.3)), (81, (0.5, 0.5, 0.5)), (81, (0.3, 0.3, 0.3))],
                         ids=["small_p0.5", "small_p0.3", "wide_p0.5", "wide_p0.3"])
def test_masked_heads_against_float64(ncls, rates):
    """T * B = 10 * 32 rows of the decoder's K = 248 features: 21 classes run the small family, 81 the wide one"""
    from rsis_amd import decoder_seq, ops
    A = _abi()
    T, B, hs = 10, 32, C.HIDS
    rows, K = T * B, sum(C.HIDS)
    assert ops.heads_family(rows, K, ncls, backward=True) == ("small" if ncls == 21 else "wide")
    d = LP.heads_normal_data((rows, hs, ncls), "normal")
    n = rows * K
    drop, (s2h, mch, msh) = _drop_of(n, rates, T, B, hs)
    # level-major flat layout: level i holds [rows][hid_i]
    flat = np.concatenate([s.reshape(-1) for s in d["sides"]])
    SIDE = dev(flat)
    Wc, bc, Ws, bs = (dev(d[k]) for k in ("Wc", "bc", "Ws", "bs"))
    probs, stop = Guarded((T, B, ncls)), Guarded((T, B, 1))
    decoder_seq._heads_fwd_masked(A.lib(), SIDE, drop, hs, T, B, Wc, bc, Ws, bs, probs.t, stop.t)
    torch.cuda.synchronize()
    side = s2h * flat                                     # one fp32 product each: the device's bits
    sc, ss = mch * side, msh * side
    for name, got, want in (("SIDE", SIDE, side), ("SIDEC", drop.SIDEC, sc), ("SIDES", drop.SIDES, ss)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), name
    assert bool((drop.SIDEC[drop.MC == 0] == 0).all()) and bool((drop.SIDES[drop.MS == 0] == 0).all())

    def levels(v):
        return [a.reshape(rows, h) for a, h in zip(np.split(v, np.cumsum([rows * h for h in hs])[:-1]), hs)]

    def case(sides):
        sv = np.concatenate(sides, 1).astype(np.float64)
        lg = sv @ d["Wc"].astype(np.float64).T + d["bc"].astype(np.float64)
        ex = np.exp(lg - lg.max(1, keepdims=True))
        return dict(d, sides=sides, probs=ex / ex.sum(1, keepdims=True), stop=sv @ d["Ws"].astype(np.float64) + float(d["bs"][0]))

    dC, dS = case(levels(sc)), case(levels(ss))
    pg = probs.check("probs").cpu().double().numpy().reshape(rows, ncls)
    sg = stop.check("stop").cpu().double().numpy().reshape(rows)
    assert bool((np.abs(pg - dC["probs"]) <= W.fwd_bounds(dC)[0]).all()), "class probabilities of the masked features: %g" % np.abs(pg - dC["probs"]).max()
    assert bool((np.abs(sg - dS["stop"]) <= W.fwd_bounds(dS)[1]).all()), "stop logits of the masked features: %g" % np.abs(sg - dS["stop"]).max()
    # backward, reading the forward's probabilities
    p32 = probs.t.cpu().numpy().reshape(rows, ncls)
    fill = {k: np.random.default_rng(7).normal(0, 1, s).astype(np.float32) for k, s in (("dWc", (ncls, K)), ("dbc", (ncls,)), ("dWs", (K,)), ("dbs", (1,)))}
    hb = [Guarded(fill[k].shape, init=fill[k]) for k in ("dWc", "dbc", "dWs", "dbs")]
    DSIDE = Guarded((n,))
    dp, ds = dev(d["dprobs"]).view(T, B, ncls), dev(d["dstop"]).view(T, B, 1)
    decoder_seq._heads_bwd_masked(A.lib(), drop, hs, T, B, Wc, Ws, probs.t, dp, ds, DSIDE.t, [g.t for g in hb])
    torch.cuda.synchronize()
    rC = LP.heads_bwd64(dC["sides"], d["Wc"], d["Ws"], p32, d["dprobs"], None)
    rS = LP.heads_bwd64(dS["sides"], d["Wc"], d["Ws"], p32, None, d["dstop"])
    bC = W.bwd_bounds(dict(dC, dstop=np.zeros_like(d["dstop"])), probs=p32)
    bS = W.bwd_bounds(dict(dS, dprobs=np.zeros_like(d["dprobs"])), probs=p32)

    def flat_of(a):            # (rows, K) -> the level-major flat layout
        return np.concatenate([x.reshape(-1) for x in np.split(a, np.cumsum(hs)[:-1], 1)])

    m1, m2 = mch.astype(np.float64), msh.astype(np.float64)
    tC, tS = m1 * flat_of(rC["dside"]), m2 * flat_of(rS["dside"])
    bound = m1 * flat_of(bC["dside"]) + m2 * flat_of(bS["dside"]) + W.gamma(3) * (np.abs(tC) + np.abs(tS)) + 3 * W.DENORM
    got = DSIDE.check("dside").cpu().double().numpy()
    assert bool((np.abs(got - (tC + tS)) <= bound).all()), "dside: %g over" % (np.abs(got - (tC + tS)) - bound).max()
    assert bool((got[(mch == 0) & (msh == 0)] == 0).all()), "a feature dropped by both heads received a gradient"
    for g, k, ref, b in ((hb[0], "dWc", rC, bC), (hb[1], "dbc", rC, bC), (hb[2], "dWs", rS, bS), (hb[3], "dbs", rS, bS)):
        err = np.abs(g.check(k).cpu().double().numpy() - (fill[k].astype(np.float64) + ref[k]))
        lim = b[k] + 2 * U * (np.abs(fill[k]) + np.abs(ref[k]))          # (accumulated into a prefill: one more addition)
        assert bool((err <= lim).all()), "%s: %g over" % (k, (err - lim).max())
    # dWc / dWs are taken against the MASKED features: a dropped feature's column sees only zeros
    colC, colS = levels(mch), levels(msh)
    dWc = hb[0].t.cpu().numpy() - fill["dWc"]
    allC = np.concatenate(colC, 1)
    dead = np.where((allC == 0).all(0))[0]
    assert bool((dWc[:, dead] == 0).all())


# ======================================================================================================================
# the one-node decoder
# ======================================================================================================================
def _oracle_run(odec, feats64, T, rec, gm, B, arg=None):
    """the float64 oracle decoder over T steps with F.dropout2d / F.dropout replaced by the recorded scales, in call order.  arg (per
    level [T][B][hid] pixels): the global max-pool reads THESE pixels -- the function a run that pooled them differentiates"""
    F = torch.nn.functional
    calls = {"t": 0, "i": 0, "pool": 0}

    def pool(x, kernel_size):
        a = arg[calls["pool"]][calls["t"]].long()
        calls["pool"] += 1
        return x.flatten(2).gather(2, a.unsqueeze(-1)).unsqueeze(-1)

    def d2(x, p, training=True):
        s = rec["s2"][calls["i"]][calls["t"]].double()
        calls["i"] += 1
        return x * s.view(x.shape[0], x.shape[1], 1, 1)

    def d1(x, p, training=True):
        which = "mc" if calls["head"] == 0 else "ms"
        calls["head"] += 1
        m = torch.cat([v[calls["t"]] for v in rec[which]], 1).double()
        return x * m.reshape(x.shape)

    was = F.dropout2d, F.dropout, F.max_pool2d
    F.dropout2d, F.dropout = d2, d1
    if arg is not None:
        F.max_pool2d = pool
    try:
        hidden, steps = None, []
        for t in range(T):
            calls.update(t=t, i=0, pool=0, head=0 if odec.dropout_cls > 0 else 1)
            m, c, s, hidden = odec(feats64, hidden)
            steps.append((m.reshape(B, -1), c.reshape(B, -1), s.reshape(B, 1)))
    finally:
        F.dropout2d, F.dropout, F.max_pool2d = was
    masks, probs, stops = (torch.stack([st[k] for st in steps], 1) for k in range(3))
    return masks, probs, stops


def _loss(masks, probs, stops, gm):
    return (masks * gm.to(masks.device, masks.dtype)).sum() + (probs * probs).sum() * 20 + stops.sum()


def _decoder_case(sizes, rates, dtype, B=C.B, ncls=21, T=C.T):
    """runs the sequence node (fp32: once; bf16: on fp32 storage and on blk storage, from the same generator state) and the float64 oracle on
    the recorded scales; returns (truth, [runs]) -- bf16: ([truth of every run, pooled at the pixels that run pooled], [runs])"""
    from oracle import filler
    from oracle import rsis_oracle as O
    from rsis_amd import decoder_seq
    from rsis_amd.modules import RSIS
    kw = dict(hidden_size=C.HS, num_classes=ncls, maxseqlen=T, dropout=rates[0], dropout_cls=rates[1], dropout_stop=rates[2])
    odec = filler.fill_module(O.RSIS(mk_args(**kw)), seed=5).double()
    dec = RSIS(mk_args(dtype=dtype, **kw)).cuda()
    dec.load_state_dict({k: v.float() for k, v in odec.state_dict().items()})
    assert list(dec.state_dict().keys()) == list(odec.state_dict().keys())
    feats_cpu = [filler.tensor(9, "do.f%d" % i, (B, C.CHANS[i]) + sizes[i]) for i in range(5)]
    gm = filler.tensor(9, "do.gm", (B, T, 4 * sizes[-1][0] * sizes[-1][1]))
    runs, rec0 = [], None
    was = decoder_seq.BLK_ENABLED[0], decoder_seq.RECORD[0]
    try:
        decoder_seq.RECORD[0] = True
        for blk in ((False, True) if dtype == "bf16" else (False,)):
            decoder_seq.BLK_ENABLED[0] = blk
            decoder_seq.LAST.clear()
            dec.zero_grad()
            dec.__dict__["_drop_state"] = _state()
            feats = [f.cuda().requires_grad_() for f in feats_cpu]
            assert decoder_seq.supported(dec, feats, T) is True
            assert decoder_seq.blk_supported(dec, feats) == blk
            masks, probs, stops, _hid, _size = decoder_seq.decoder_sequence_stacked(dec, feats, T)
            for o in (masks, probs, stops):
                assert "_DecoderSeqFn" in type(o.grad_fn).__name__, "the outputs do not come from the sequence node: %r" % o.grad_fn
            _loss(masks, probs, stops, gm).backward()
            rec = {k: ([x.cpu() for x in v] if v is not None else None) for k, v in decoder_seq.LAST["drop"].items()}
            if rec0 is not None:
                assert all(torch.equal(a, b) for k in ("mc", "ms") for a, b in zip(rec0[k], rec[k])), "the same state drew other masks"
            rec0 = rec
            runs.append(([o.detach().cpu().double() for o in (masks, probs, stops)], [f.grad.cpu().double() for f in feats],
                         {k: p.grad.cpu().double() for k, p in dec.named_parameters()}, [a.cpu() for a in decoder_seq.LAST["arg"]]))
    finally:
        decoder_seq.BLK_ENABLED[0], decoder_seq.RECORD[0] = was
        decoder_seq.LAST.clear()
    # the recorded scales are the numpy rule's at the tests' state
    want = C.masks(C.state0(), rates, T, B)
    for name, a, w in (("s2", rec0["s2"], want[0]), ("mc", rec0["mc"], want[1]), ("ms", rec0["ms"], want[2])):
        if a is None:
            assert rates[0] == 0
            continue
        assert np.array_equal(np.concatenate([x.numpy().reshape(-1) for x in a]), w), name
    def truth_at(arg):
        odec.zero_grad()
        f64 = [f.double().requires_grad_() for f in feats_cpu]
        om, op, os_ = _oracle_run(odec, f64, T, rec0, gm, B, arg)
        _loss(om, op, os_, gm.double()).backward()
        return [om.detach(), op.detach(), os_.detach()], [f.grad for f in f64], {k: p.grad.clone() for k, p in odec.named_parameters()}

    if dtype != "bf16":
        return truth_at(None), runs
    same = all(torch.equal(a, b) for a, b in zip(runs[0][3], runs[1][3]))
    t0 = truth_at(runs[0][3])
    return [t0, t0 if same else truth_at(runs[1][3])], runs


def _check_fp32(truth, run):
    for name, got, ref in zip(("masks", "class probs", "stop"), run[0], truth[0]):
        assert_close(name, got, ref, 1e-4)
    for name, got, ref in ([("dfeat%d" % i, run[1][i], truth[1][i]) for i in range(5)] + [("grad." + k, run[2][k], truth[2][k]) for k in truth[2]]):
        assert_close(name, got, ref, 1e-4 * max(1.0, float(ref.abs().max())))


def _check_blk(truths, runs):
    """the bars of test_gpu_blk_dec.py between blk and fp32 storage.  The global max-pool is not continuous: where the two storage formats
    pool ANOTHER pixel of a plane (a near-tie decided by a bf16 rounding; tools/exp/bf16_flip_diag.py), they differentiate different
    functions from that level down -- the gradient reaches level i from the levels above it only through h[i].  So every run is held to
    the float64 oracle pooled at the pixels THAT run pooled, and the two runs are compared with each other on the tensors no differing
    plane can reach: all of them when there is none (asserted to be the common case: at most 1 % of the planes of a level)."""
    rel = lambda x, y: float((x - y).norm() / y.norm().clamp_min(1e-30))
    flips = [int((a != b).sum()) for a, b in zip(runs[0][3], runs[1][3])]
    print("planes pooled at another pixel, per level:", flips)
    assert all(f <= max(1, a.numel() // 100) for f, a in zip(flips, runs[0][3])), flips
    reach = max([i for i, f in enumerate(flips) if f] or [-1])            # levels 0 .. reach see a differing plane
    for name, r0, r1 in zip(("masks", "class probs", "stop"), runs[0][0], runs[1][0]):
        assert float((r1 - r0).abs().max()) <= 0.02 * float(r0.abs().max()), "%s: %g of max" % (name, float((r1 - r0).abs().max() / r0.abs().max()))
    level = lambda k: int(k.split(".")[1]) if k.startswith("clstm_list.") else 99
    for name, lv, r0, r1, t0, t1 in ([("dfeat%d" % i, i, runs[0][1][i], runs[1][1][i], truths[0][1][i], truths[1][1][i]) for i in range(5)] +
                                     [("grad." + k, level(k), runs[0][2][k], runs[1][2][k], truths[0][2][k], truths[1][2][k]) for k in truths[0][2]]):
        e_store, e0, e1 = rel(r1, r0), rel(r0, t0), rel(r1, t1)
        print("%-32s blk vs fp32 storage %.4f, fp32 storage vs float64 %.4f, blk vs float64 %.4f" % (name, e_store, e0, e1))
        if lv > reach:
            assert e_store <= 0.06, "%s: blk storage is %.3f relative L2 from the fp32-storage path" % (name, e_store)
        assert e1 <= 1.5 * e0 + 0.01, "%s: %.4f from float64 (fp32 storage: %.4f)" % (name, e1, e0)


RATES = {"dropout": (0.5, 0.0, 0.0), "cls": (0.0, 0.5, 0.0), "stop": (0.0, 0.0, 0.5), "all": (0.5, 0.5, 0.5), "all_p0.3": (0.3, 0.3, 0.3)}
DEC_CASES = [("pow2", "dropout"), ("pow2", "cls"), ("pow2", "stop"), ("pow2", "all"), ("odd", "all"), ("same", "all"), ("odd", "all_p0.3")]


@pytest.mark.parametrize("sizes,rates", DEC_CASES, ids=["%s-%s" % c for c in DEC_CASES])
def test_decoder_fp32_against_the_oracle_on_the_recorded_scales(sizes, rates):
    truth, runs = _decoder_case(C.SIZES[sizes], RATES[rates], "fp32")
    _check_fp32(truth, runs[0])


@pytest.mark.parametrize("sizes,rates", DEC_CASES, ids=["%s-%s" % c for c in DEC_CASES])
def test_decoder_blk_bf16_against_fp32_storage_and_the_oracle(sizes, rates):
    truth, runs = _decoder_case(C.SIZES[sizes], RATES[rates], "bf16")
    _check_blk(truth, runs)


@pytest.mark.parametrize("B,ncls", [(1, 21), (2, 81)], ids=["batch_1", "81_classes"])
def test_decoder_fp32_at_batch_one_and_on_the_wide_heads(B, ncls):
    truth, runs = _decoder_case(C.SIZES["odd"], RATES["all"], "fp32", B=B, ncls=ncls)
    _check_fp32(truth, runs[0])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dropped_planes_and_features_receive_exactly_zero(dtype):
    """B = 1, T = 1: h[i][0] feeds only its upsample and its pooled feature, so a plane with s2 = 0 has dh = 0 exactly -- the four gate rows
    of its channel get a zero weight and bias gradient (a kept one does not); a head feature with mask 0 gives its column of fc_class /
    fc_stop a zero gradient"""
    from oracle import filler
    from rsis_amd import decoder_seq
    from rsis_amd.modules import RSIS
    kw = dict(hidden_size=C.HS, maxseqlen=1, dropout=0.5, dropout_cls=0.5, dropout_stop=0.5, dtype=dtype)
    dec = filler.fill_module(RSIS(mk_args(**kw)), seed=5).cuda()
    dec.__dict__["_drop_state"] = _state()
    feats = [filler.tensor(9, "dz.f%d" % i, (1, C.CHANS[i]) + C.SIZES["same"][i]).cuda().requires_grad_() for i in range(5)]
    assert decoder_seq.supported(dec, feats, 1) and decoder_seq.blk_supported(dec, feats) == (dtype == "bf16")
    masks, probs, stops, _hid, _size = decoder_seq.decoder_sequence_stacked(dec, feats, 1)
    gm = filler.tensor(9, "dz.gm", tuple(masks.shape)).cuda()
    _loss(masks, probs, stops, gm).backward()
    s2, mc, ms = C.masks(C.state0(), (0.5, 0.5, 0.5), 1, 1)
    for i, (cell, s) in enumerate(zip(dec.clstm_list, C.per_level(s2, 1, 1))):
        hid = C.HIDS[i]
        gw, gb = cell.Gates.weight.grad.view(4, hid, -1), cell.Gates.bias.grad.view(4, hid)
        dropped = torch.from_numpy(s[0, 0] == 0).cuda()
        assert bool(dropped.any()) and bool((~dropped).any())
        assert bool((gw[:, dropped] == 0).all()) and bool((gb[:, dropped] == 0).all()), "level %d: a dropped plane's gate rows have a gradient" % i
        assert bool((gw[:, ~dropped].abs().amax((0, 2)) > 0).all()), "level %d: a kept plane's gate rows have none" % i
    mcat = lambda m: torch.from_numpy(np.concatenate([v[0, 0] for v in C.per_level(m, 1, 1)])).cuda()
    assert bool((dec.fc_class.weight.grad[:, mcat(mc) == 0] == 0).all()) and bool((dec.fc_class.weight.grad[:, (mcat(mc) > 0) & (mcat(s2) > 0)] != 0).any())
    assert bool((dec.fc_stop.weight.grad[:, mcat(ms) == 0] == 0).all())


# ======================================================================================================================
# all rates 0: today's path
# ======================================================================================================================
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_dropout_touches_no_generator_and_keeps_its_bits(dtype):
    from oracle import filler
    from rsis_amd import decoder_seq
    from rsis_amd.modules import RSIS
    T = C.T
    dec = filler.fill_module(RSIS(mk_args(hidden_size=C.HS, maxseqlen=T, dtype=dtype)), seed=5).cuda()
    feats_cpu = [filler.tensor(9, "dn.f%d" % i, (C.B, C.CHANS[i]) + C.SIZES["odd"][i]) for i in range(5)]

    def run(d):
        d.zero_grad()
        feats = [f.cuda().requires_grad_() for f in feats_cpu]
        masks, probs, stops, _hid, _size = decoder_seq.decoder_sequence_stacked(d, feats, T)
        gm = filler.tensor(9, "dn.gm", tuple(masks.shape)).cuda()
        _loss(masks, probs, stops, gm).backward()
        return [masks.detach(), probs.detach(), stops.detach()] + [f.grad for f in feats]

    from rsis_amd import ops
    prev = ops.set_deterministic(True)          # (bit-equal runs need the library's fixed-order reductions)
    try:
        _no_dropout_body(dec, other_args=dict(hidden_size=C.HS, maxseqlen=T, dtype=dtype, dropout=0.5, dropout_cls=0.5, dropout_stop=0.5), run=run)
    finally:
        ops.set_deterministic(prev)


def _no_dropout_body(dec, other_args, run):
    from oracle import filler
    from rsis_amd import decoder_seq
    from rsis_amd.modules import RSIS
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    was = decoder_seq.RECORD[0]
    decoder_seq.RECORD[0] = True
    decoder_seq.LAST.clear()
    try:
        first = run(dec)
        assert "arg" in decoder_seq.LAST and "drop" not in decoder_seq.LAST, "a scale buffer was made at rate 0"
    finally:
        decoder_seq.RECORD[0] = was
        decoder_seq.LAST.clear()
    assert "_drop_state" not in dec.__dict__
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0), "a torch generator was advanced at rate 0"
    # now a decoder WITH dropout draws (key from torch's generator, device state), then the first one again
    other = filler.fill_module(RSIS(mk_args(**other_args)), seed=5).cuda()
    a, b = run(other), run(other)
    assert "_drop_state" in other.__dict__ and sorted(other.state_dict()) == sorted(dec.state_dict()), "the state must not be a state_dict key"
    assert not torch.equal(a[0], b[0]), "two sequences of a dropout decoder drew the same masks"
    assert not torch.equal(torch.get_rng_state(), cpu0), "the key was not taken from torch's seeded generator"
    again = run(dec)
    for x, y in zip(first, again):
        assert torch.equal(_bits(x), _bits(y))


# ======================================================================================================================
# hipGraph
# ======================================================================================================================
@pytest.mark.parametrize("extra", [[], ["-dtype", "bf16"]], ids=["fp32", "bf16"])
def test_train_py_graph_replays_with_fresh_masks(extra, tmp_path):
    """one resident synthetic batch, learning rates 0: every epoch is the same iteration on the same weights, so the epoch's training loss
    moves only with the masks.  Epochs 0-1 run eagerly, 2 captures, 3.. replay."""
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "rsis_amd.train", "--synthetic", "--graph", "-imsize", "64", "-batch_size", "2", "-maxseqlen", "3",
           "-gt_maxseqlen", "4", "-dropout", "0.5", "-dropout_cls", "0.5", "-dropout_stop", "0.5", "--log_term", "-synthetic_batches", "1", "-max_epoch", "6",
           "-lr", "0", "-lr_cnn", "0", "-weight_decay", "0", "-weight_decay_cnn", "0", "--use_class_loss", "--use_stop_loss", "-print_every", "1",
           "-models_root", str(tmp_path / "models"), "-model_name", "drop"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "capture failed" not in out and "per-step-decoder" not in out and "decoder runs per step" not in out, out[-3000:]
    totals = [float(l.split("total:")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("Epoch") and "(train)" in l]
    assert len(totals) == 6 and all(np.isfinite(totals)), out[-3000:]
    assert totals[3] != totals[4] and totals[4] != totals[5], "consecutive replays report the same loss: %s" % totals
