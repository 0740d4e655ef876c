"""Cases, float64 references and bars of the weight-gradient lane tests (tests/test_gpu_wgrad_lanes.py on the device,
tests/test_wgrad_lane_bars_host.py for the bars themselves).  Plain Python: nothing here needs a GPU.

A CASE is one dW and the jobs (rsis_wgrad_job) that accumulate into it: the sources of a concat write disjoint columns, the five jobs
of `same_dw` write the same elements, the ConvLSTM pair reads one dy stack at two image offsets.  A CALL is a list of cases that go
into ONE rsis_conv2d_wgrad_batch call.  In default mode (rsis_conv2d_wgrad_batch, api.hip: `!rsis_deterministic()` in front of
"grouped below") the bf16 / blk jobs of a call are bucketed by kernel instantiation (wgb_key) and every bucket is planned by
wgb_plan_lanes with L = max(2, ceil(bucket's (dW tile, spatial tile) pairs / 896)) spatial tiles per block.

Families: "bf16" = RSIS_DTYPE_BF16 (fp32 storage, the register-staged kernels), "blk" = RSIS_DTYPE_BF16_BLK (channel-blocked bf16
operands, the DMA kernels).  Per family the calls are
  base      the instantiation list: _C3 + _C1 of test_gpu_wgrad_staged.py / the blk list of test_gpu_wgrad_paths.py
  splits    23 one-tile images: 12 splits at L = 2, the last a single tile, eight items of 1, 2, 1, 2, 1, 2, 1, 2 splits; 3x3 and 1x1
  pad       a one-tile job next to large ones (the issue's pair, and a six-tile job of the one-tile job's own instantiation, so that
            the two share a launch: the one-tile item leaves padding blocks in the other lanes)
  many      40 one-tile jobs: 32 in the first launch, 8 in the second
  items     29 jobs of 8 items: 232 > 8 * 28, the first launch ends at 28 jobs, both launches cut by the same total
  same_dw   five jobs, their own dy / x, into the same dW elements
  lstm_pair the ConvLSTM weight as rsis_amd/decoder_fused.py issues it: hid 16, c_up 24, 7 x 7, B = 2, n = 3 steps; job A 6 images of
            the 24 `up` channels at c_off 0, job B dy from image 2 on with 4 images of the 16 state channels at c_off 24; Ctot = 40
  inf       one +inf in x, 3x3 and 1x1
  all       every case above in ONE call, as ops.flush_wgrads sends the layers of a step (the lane-specific calls above keep their own
            calls as well: the launches they are named for depend on what else is in their bucket)
and one call `mixed` holds fp32 tiled, fp32 staged-limb, bf16, blk, a stride-2 3x3 and a Cout == 1 job in shuffled order.

Reference: float64 autograd of F.conv2d on operands rounded to bf16 by torch.bfloat16() (round to nearest even; fp32 jobs: not
rounded), plus the pre-filled dW.

Bars, stated before anything ran:
  TIGHT     (default mode: a block walks ~2 tiles) what the family's single-launch test already asks:
            bf16  atol 4e-6 * max(sqrt(n), max |g|) + 1e-6, rtol 1e-5      (test_bf16_conv2d_fwd_bwd_exact_semantics; n = B H W of a job)
            blk   atol 2e-5 * max |g|, rtol 1e-4                           (test_blk_conv_weight_gradient)
            k jobs into one element: k times the atol.  g: the gradient without the pre-filled contents; rtol counts on |prev + g|.
  ROUNDING  (a block walks many tiles: deterministic mode, RSIS_WGB_GROUP_BLOCKS=8) the worst case of ANY fp32 summation of exactly
            representable terms, derived, not measured: |err_ij| <= n 2^-23 (|prev_ij| + A_ij), A the float64 weight gradient of
            |dy|, |x|, n = B H W summed over the jobs that write the element.
  fp32 jobs (only in `mixed`): 2e-5 * max(1, max |ref|), the bar test_conv2d_wgrad_fp32_on_ragged_maps and
            test_gpu_wgrad_staged.py ask in default and in deterministic mode alike; it stands for TIGHT and for ROUNDING."""
import collections
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
from test_gpu_wgrad_paths import CASES as _PATHS_CASES  # noqa: E402
from test_gpu_wgrad_staged import _C1, _C3, _inf_mask  # noqa: E402

FAMILIES = ("bf16", "blk")
INF_AT = (1, 5, 7, 9)        # (image, channel, y, x) of the +inf, as in test_gpu_wgrad_staged.py
WGB_MAXJ, WGB_LANE_ITEMS, WGB_TARGET = 32, 28, 896      # RSIS_WGB_MAXJ, RSIS_WGB_LANE_ITEMS (wgrad_lanes.h); target_blocks (wgb_launch_bucket)

Job = collections.namedtuple("Job", "B Cs c_off dy img0")      # dy: index into the case's dy stacks; img0: first image of it the job reads


class Case(object):
    """one dW (Cout, Ctot, ks, ks) and its jobs; ndy[i] = images of dy stack i"""

    def __init__(self, name, dtype, H, W, Cout, Ctot, ks, hid, jobs, ndy, seed, stride=1, kind=""):
        self.name, self.dtype, self.H, self.W, self.Cout, self.Ctot, self.ks, self.hid = name, dtype, H, W, Cout, Ctot, ks, hid
        self.jobs, self.ndy, self.seed, self.stride, self.kind = jobs, ndy, seed, stride, kind
        self.pad = ks // 2
        self.Ho, self.Wo = (H + 2 * self.pad - ks) // stride + 1, (W + 2 * self.pad - ks) // stride + 1

    def __repr__(self):
        return "%s[%s %dx%d Cout %d ks %d%s%s jobs %r]" % (self.name, self.dtype, self.H, self.W, self.Cout, self.ks,
                                                           " s%d" % self.stride if self.stride > 1 else "",
                                                           " hid %d" % self.hid if self.hid else "", [tuple(j) for j in self.jobs])


_seed = [0]


def _case(name, dtype, t, kind="", stride=1):
    """(B, [Cin segs], H, W, Cout, ks, hid) -> a case: one dy stack, one job per source"""
    B, segs, H, W, Cout, ks, hid = t[:7]
    _seed[0] += 1
    jobs, off = [], 0
    for c in segs:
        jobs.append(Job(B, c, off, 0, 0))
        off += c
    return Case(name, dtype, H, W, Cout, off, ks, hid, jobs, [B], _seed[0], stride, kind)


def _same_dw(name, dtype):
    _seed[0] += 1
    return Case(name, dtype, 16, 16, 32, 32, 3, 0, [Job(2, 32, 0, i, 0) for i in range(5)], [2] * 5, _seed[0])


def _lstm_pair(name, dtype):
    hid, c_up, B, n = 16, 24, 2, 3
    _seed[0] += 1
    return Case(name, dtype, 7, 7, 4 * hid, c_up + hid, 3, hid, [Job(n * B, c_up, 0, 0, 0), Job((n - 1) * B, hid, c_up, 0, B)], [n * B], _seed[0])


def _family_calls(f):
    base = _C3 + _C1 if f == "bf16" else _PATHS_CASES["blk"]
    one = (1, [32], 8, 8, 32, 3, 0)
    calls = collections.OrderedDict()
    calls[f + "/base"] = [_case("%s/base%d" % (f, k), f, t) for k, t in enumerate(base)]
    calls[f + "/splits"] = [_case(f + "/splits3", f, (23, [32], 8, 8, 32, 3, 0)), _case(f + "/splits1", f, (23, [32], 8, 8, 64, 1, 0))]
    calls[f + "/pad"] = [_case(f + "/pad_one", f, one), _case(f + "/pad_large", f, (4, [64], 16, 16, 64, 3, 0)),
                         _case(f + "/pad_six", f, (6, [32], 8, 8, 32, 3, 0))]
    calls[f + "/many"] = [_case("%s/many%d" % (f, k), f, one) for k in range(WGB_MAXJ + 8)]
    calls[f + "/items"] = [_case("%s/items%d" % (f, k), f, (16, [32], 8, 8, 32, 3, 0)) for k in range(29)]
    calls[f + "/same_dw"] = [_same_dw(f + "/same_dw", f)]
    calls[f + "/lstm_pair"] = [_lstm_pair(f + "/lstm_pair", f)]
    calls[f + "/inf"] = [_case(f + "/inf3", f, (2, [64], 16, 16, 64, 3, 0), "inf"), _case(f + "/inf1", f, (2, [64], 16, 16, 64, 1, 0), "inf")]
    calls[f + "/all"] = [c for cs in calls.values() for c in cs]      # the same cases, the whole family in ONE call
    return calls


def _mixed():
    c = [
        _case("mixed/f32_tiled1", "f32", (2, [64], 8, 32, 96, 1, 0)), _case("mixed/f32_tiled3", "f32", (2, [16], 16, 16, 32, 3, 0)),
        _case("mixed/f32_staged5", "f32", (2, [32], 4, 32, 64, 3, 0)),        # wgl_class 5: Cs % 32 == 0, 32-wide tiles, Cout <= 64
        _case("mixed/f32_staged2", "f32", (2, [32], 4, 32, 72, 3, 0)),        # wgl_class 2: the same with Cout > 64
        _case("mixed/bf16_1a", "bf16", (3, [40], 7, 7, 48, 1, 0)), _case("mixed/bf16_1b", "bf16", (2, [136], 16, 16, 264, 1, 0)),
        _case("mixed/bf16_3a", "bf16", (2, [40], 8, 8, 24, 3, 0)), _case("mixed/bf16_3b", "bf16", (2, [72], 5, 13, 200, 3, 0)),
        _case("mixed/blk_1", "blk", (2, [64], 8, 8, 136, 1, 0)), _case("mixed/blk_3", "blk", (3, [40], 14, 14, 24, 3, 0)),
        _case("mixed/f32_stride2", "f32", (2, [24], 16, 24, 40, 3, 0), stride=2),      # the generic split-K kernel
        _case("mixed/f32_cout1", "f32", (2, [16], 16, 16, 1, 3, 0)),                   # conv_c1
    ]
    return c


def wgl_class(c, job):
    """wgl_class of conv_wgrad_bf16.hip, restated (the fp32 jobs of `mixed` that the default table sends to the staged limb kernels)"""
    if c.ks == 3:
        twi = 2 if c.W > 16 else (1 if c.W > 8 else 0)
        tw = 8 << twi
        if job.Cs % 32 or c.W % tw or c.H % (64 // tw):
            return -1
        return (0 if c.Cout > 64 else 3) + twi
    if (c.H * c.W) % 64 or c.Cout <= 32:
        return -1
    return 6 if (c.Cout >= 128 and job.Cs >= 128) else 7


CALLS = collections.OrderedDict()
for _f in FAMILIES:
    CALLS.update(_family_calls(_f))
CALLS["mixed"] = _mixed()
MIXED_ORDER = [7, 2, 10, 0, 9, 4, 11, 1, 6, 3, 8, 5]       # the order of the mixed call's jobs (one job per case), fixed
assert sorted(MIXED_ORDER) == list(range(len(CALLS["mixed"])))
ALL_CASES = [c for call, cs in CALLS.items() if not call.endswith("/all") for c in cs]


def family_of(call):
    return call.split("/")[0]


# ---- the dispatch rule (wgb_key of conv_wgrad_bf16.hip), restated so that a retuned rule is seen to leave cases behind
def w3t_th(bm, tw):
    """tile height of the blk 3x3 DMA kernel"""
    if tw == 32:
        return 2 if bm == 128 else 4
    if tw == 16:
        return 4 if bm == 128 else 8
    return 8


def wgb_key(c, job):
    """(ks, bm, bn, tw, th, v4) of one job; 1x1 runs on the flattened map, 64 pixels per tile; v4: 2 blk, else whole-float4 loads"""
    blk = c.dtype == "blk"
    if c.ks == 3:
        tw = 32 if c.W > 16 else (16 if c.W > 8 else 8)
        bm = 32 if c.Cout <= 32 else (64 if (c.Cout <= 64 or job.Cs <= 512) else 128)
        return (3, bm, 32, tw, w3t_th(bm, tw) if blk else 64 // tw, 2 if blk else int(c.W % 4 == 0))
    return (1, 64 if c.Cout <= 64 else 128, 64 if job.Cs <= 64 else 128, 64, 1, 2 if blk else int((c.H * c.W) % 4 == 0))


def instantiations(c):
    """bf16: (3, BM, TW, aligned) / (1, BM, BN, aligned); blk: (3, BM, TW) / (1, BM, BN)"""
    out = set()
    for j in c.jobs:
        ks, bm, bn, tw, th, v4 = wgb_key(c, j)
        k = (3, bm, tw) if ks == 3 else (1, bm, bn)
        out.add(k if c.dtype == "blk" else k + (bool(v4),))
    return out


def all_instantiations(f):
    k = {(3, bm, tw) for bm in (32, 64, 128) for tw in (8, 16, 32)} | {(1, bm, bn) for bm in (64, 128) for bn in (64, 128)}
    return k if f == "blk" else {i + (v,) for i in k for v in (False, True)}


def _cdiv(a, b):
    return -(-a // b)


def spatial_tiles(c, job):
    ks, bm, bn, tw, th, v4 = wgb_key(c, job)
    return job.B * _cdiv(c.H * c.W, 64) if ks == 1 else job.B * _cdiv(c.H, th) * _cdiv(c.W, tw)


def dw_tiles(c, job):
    ks, bm, bn, tw, th, v4 = wgb_key(c, job)
    return _cdiv(c.Cout, bm) * _cdiv(job.Cs, bn)


def lane_splits(call, target):
    """splits of every bf16 / blk job of a grouped call as wgb_plan_lanes cuts them at `target` blocks (a bucket = the jobs of one
    instantiation; every block walks L = max(2, ceil(bucket's tile pairs / target)) spatial tiles): {case name: [splits per job]}"""
    total = collections.defaultdict(int)
    for c in CALLS[call]:
        for j in c.jobs:
            total[(c.dtype,) + wgb_key(c, j)] += dw_tiles(c, j) * spatial_tiles(c, j)
    out = {}
    for c in CALLS[call]:
        if c.dtype in FAMILIES:
            out[c.name] = []
            for j in c.jobs:
                L = max(2, _cdiv(total[(c.dtype,) + wgb_key(c, j)], target))
                sp = spatial_tiles(c, j)
                out[c.name].append(_cdiv(sp, _cdiv(sp, max(1, _cdiv(sp, L)))))
    return out


# ---- inputs and the float64 reference
def _rng_t(seed, i, shape):
    return torch.from_numpy(np.random.default_rng([seed, i]).normal(0, 1.0, shape).astype(np.float32))


def inputs(c):
    """seeded N(0, 1): (dy stacks in the reference's row order, one x per job, the pre-filled dW)"""
    dys = [_rng_t(c.seed, i, (n, c.Cout, c.Ho, c.Wo)) for i, n in enumerate(c.ndy)]
    xs = [_rng_t(c.seed, 100 + i, (j.B, j.Cs, c.H, c.W)) for i, j in enumerate(c.jobs)]
    if c.kind == "inf":
        xs[0][INF_AT] = float("inf")
    return dys, xs, _rng_t(c.seed, 999, (c.Cout, c.Ctot, c.ks, c.ks))


def rne(t):
    return t.bfloat16().double()


def truncated(t):
    """fp32 -> bf16 by dropping the low 16 bits (what a kernel that does not round would do)"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def wgrad64(c, dy, x):
    w = torch.zeros(c.Cout, x.shape[1], c.ks, c.ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, stride=c.stride, padding=c.pad).backward(dy)
    return w.grad


def inf_mask(c):
    """dW elements whose reduction contains the +inf (_inf_mask of the staged test)"""
    return _inf_mask((c.jobs[0].B, [c.Ctot], c.H, c.W, c.Cout, c.ks, c.hid, c.kind))


def gradient(c, ins=None, rnd=None, edit=None):
    """float64 sum of the jobs' weight gradients (without prev).  rnd: the rounding of the operands (default: the case's own);
    edit(k, dy, x) -> dy: changes the dy a job sees (the wrong results of the host test)"""
    dys, xs, prev = ins if ins is not None else inputs(c)
    rnd = rnd or ((lambda t: t.double()) if c.dtype == "f32" else rne)
    g = torch.zeros(c.Cout, c.Ctot, c.ks, c.ks, dtype=torch.float64)
    for k, (j, x) in enumerate(zip(c.jobs, xs)):
        x = x.clone()
        if c.kind == "inf" and k == 0:        # the reduction that contains the inf is masked (inf_mask); the rest is the finite sum
            x[INF_AT] = 0.0
        dy = rnd(dys[j.dy][j.img0:j.img0 + j.B])
        if edit is not None:
            dy = edit(k, dy)
        g[:, j.c_off:j.c_off + j.Cs] += wgrad64(c, dy, rnd(x))
    return g


_REF = {}


def reference(c):
    """dict: prev, g (the gradient without prev), ref = prev + g, A (gradient of |dy|, |x|), n (B H W summed over the jobs that write
    the element), k (jobs that write the element), mask (reductions that contain the inf); float64, computed once"""
    if c.name not in _REF:
        ins = inputs(c)
        dys, xs, prev = ins
        g = gradient(c, ins)
        absr = (lambda t: t.double().abs()) if c.dtype == "f32" else (lambda t: rne(t).abs())
        A = gradient(c, ins, rnd=absr)
        n, k = torch.zeros_like(g), torch.zeros_like(g)
        for j in c.jobs:
            n[:, j.c_off:j.c_off + j.Cs] += j.B * c.Ho * c.Wo
            k[:, j.c_off:j.c_off + j.Cs] += 1
        assert float(k.min()) >= 1
        _REF[c.name] = dict(prev=prev.double(), g=g, ref=prev.double() + g, A=A, n=n, k=k, mask=inf_mask(c))
    return _REF[c.name]


# ---- bars: the allowed |got - ref| per element
def _f32_bar(R):
    return torch.full_like(R["ref"], 2e-5 * max(1.0, float(R["ref"].abs().max())))


def tight(c, R):
    if c.dtype == "f32":
        return _f32_bar(R)
    gmax = float(R["g"].abs().max())
    if c.dtype == "bf16":
        n_job = R["n"] / R["k"]
        return R["k"] * (4e-6 * torch.clamp(n_job.sqrt(), min=gmax) + 1e-6) + 1e-5 * R["ref"].abs()
    return R["k"] * 2e-5 * gmax + 1e-4 * R["ref"].abs()


def rounding(c, R):
    if c.dtype == "f32":
        return _f32_bar(R)
    return R["n"] * 2.0 ** -23 * (R["prev"].abs() + R["A"])


BARS = {"TIGHT": tight, "ROUNDING": rounding}


def ratio(c, got, bar):
    """worst |got - ref| / bar over the elements whose reduction holds no inf (inf where a result is not finite); the element"""
    R = reference(c)
    err = (got.double() - R["ref"]).abs() / BARS[bar](c, R)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    err = torch.where(R["mask"], torch.zeros_like(err), err)
    i = int(torch.argmax(err))
    return float(err.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, err.shape))


def check(what, c, got, bar, factor=1.0):
    """assert |got - ref| <= bar per element through helpers.assert_close (so that RSIS_TEST_MARGINS records err / bar): the
    comparison is of err / bar against 0 with atol 1; returns err / bar"""
    from helpers import assert_close
    R = reference(c)
    assert got.shape == R["ref"].shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(R["ref"].shape))
    tol = BARS[bar](c, R) * factor
    d = got.double() - R["ref"]
    d = torch.where(R["mask"], torch.zeros_like(d), d)
    r, at = ratio(c, got, bar)
    assert_close("%s %r %s: |err| / bar (worst %.3g at %s: got %.6g want %.6g bar %.3e)"
                 % (what, c, bar, r, at, float(got[at]), float(R["ref"][at]), float(tol[at])), d / tol, torch.zeros_like(d), 1.0)
    return r


# ---- wrong results built from the reference alone (tests/test_wgrad_lane_bars_host.py)
def _tile_masks(c):
    """dy masks (B, 1, Ho, Wo) of job 0: one spatial tile of one image; the tiles of one split at L = 2 (two tiles in the order
    (image, tile row, tile column); a job of one tile: that tile)"""
    j = c.jobs[0]
    ks, bm, bn, tw, th, v4 = wgb_key(c, j)
    one, two = torch.zeros(j.B, 1, c.Ho * c.Wo), torch.zeros(j.B, 1, c.Ho * c.Wo)
    if ks == 1:
        tiles = [(b, slice(64 * t, 64 * (t + 1))) for b in range(j.B) for t in range(_cdiv(c.Ho * c.Wo, 64))]
        one[tiles[-1][0], :, tiles[-1][1]] = 1
        for b, s in tiles[:2]:
            two[b, :, s] = 1
        return one.reshape(j.B, 1, c.Ho, c.Wo), two.reshape(j.B, 1, c.Ho, c.Wo)
    one, two = one.reshape(j.B, 1, c.Ho, c.Wo), two.reshape(j.B, 1, c.Ho, c.Wo)
    tiles = [(b, slice(th * y, th * (y + 1)), slice(tw * x, tw * (x + 1))) for b in range(j.B) for y in range(_cdiv(c.Ho, th))
             for x in range(_cdiv(c.Wo, tw))]
    b, ys, xs = tiles[-1]
    one[b, :, ys, xs] = 1
    for b, ys, xs in tiles[:2]:
        two[b, :, ys, xs] = 1
    return one, two


WRONG = ("tile_left_out", "split_twice", "taps_transposed", "truncated")


def wrong_result(c, how):
    """a dW that a subtly wrong kernel would give, float64, from the reference's own arithmetic"""
    R = reference(c)
    if how == "truncated":
        assert c.dtype != "f32"
        return R["prev"] + gradient(c, rnd=truncated)
    if how == "taps_transposed":
        assert c.ks == 3
        return R["prev"] + R["g"].transpose(2, 3)
    one, two = _tile_masks(c)
    m = (one if how == "tile_left_out" else two).double()
    part = gradient(c, edit=lambda k, dy: dy * m if k == 0 else torch.zeros_like(dy))
    return R["ref"] - part if how == "tile_left_out" else R["ref"] + part
