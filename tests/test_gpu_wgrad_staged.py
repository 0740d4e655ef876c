"""fp32 weight gradients on the STAGED limb kernels (LIMBS = 1 of wgrad3_bf16_body / wgrad1_bf16_body, rsis_amd/csrc/conv_wgrad_bf16.hip:
every staged element split once into three exact bf16 limbs, six limb products per K16 step) against FLOAT64 autograd of F.conv2d
(nn.Conv2d of reference src/modules/clstm.py:17,44), next to the exact-f32 loop and the register-split limb loop of
conv_wgrad_tiled.hip on the same inputs.  Bars, stated from the project's existing ones before the kernel ran:

  * with e32 = error of the f32 loop and e_reg = error of the register-split loop on the same case, the staged result's error el
    satisfies el <= 2 * max(e32, e_reg) (the rule tests/test_gpu_wino.py and tests/test_gpu_wgrad_limbs.py apply to a changed
    arithmetic; the products are the register-split loop's six) and el <= 2e-5 * max(1, max |ref|) (the bar of
    test_conv2d_wgrad_fp32_on_ragged_maps);
  * a single +inf in x: exactly the dW elements whose reduction contains it are non-finite, under RSIS_WGRAD_LIMBS=0 and =staged
    alike, and the rest stay inside the bars;
  * RSIS_WGRAD_LIMBS=staged in deterministic mode: two calls give equal bits, and they are the parent build's bits (against a dump
    the parent build wrote, single and grouped; skipped when there is none);
  * the default against RSIS_WGRAD_LIMBS=reg, both in deterministic mode: equal bits on every case (deterministic mode does not
    reroute);
  * under RSIS_WGRAD_LIMBS=staged a stride-2 3x3 and a Cout == 1 job return RSIS_ERR_UNSUPPORTED (no silent fallback), so every call
    that succeeds there has run the staged kernels.  No case is skipped or filtered.

RSIS_WGRAD_LIMBS is read once per process: `0`, `all`, `staged` and `reg` run in child processes (this file, as a script), one after
the other, none started after one fails; the default (the measured table) runs in the test process.  Every case runs as single
launches and in one grouped call, each on top of a pre-filled dW.

The dispatch rule of the staged kernels (wgb_key), restated so that a retuned rule is seen to leave cases behind -- _instantiation()
below computes it and test_every_instantiation_has_a_case checks the list against it:
  3x3: tile width 32 if W > 16, 16 if W > 8, else 8; dy rows per block BM = 32 if Cout <= 32, 64 if Cout <= 64 or Cs <= 512, else
       128; whole-float4 loads iff W % 4 == 0                                   -> 3 x 3 x 2 instantiations
  1x1: the flattened map; BM = 64 if Cout <= 64 else 128; BN = 64 if Cs <= 64 else 128; whole-float4 loads iff H * W % 4 == 0
                                                                                -> 2 x 2 x 2 instantiations
Shapes are the smallest at which the kernels can go wrong (B <= 4, maps <= 32 x 32): channel counts that are no multiples of the
32-channel slab or of the tile, gate convs with gate-interleaved dy rows, ragged maps, 1 / 2 / 3 spatial tiles per block (one stage,
no second buffer: every branch of the load / store / barrier sequence), and a grouped call of more jobs than one launch holds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 3
WGB_MAXJ = 32       # RSIS_WGB_MAXJ of wgrad_lanes.h: jobs per grouped launch

# (B, [Cin segs], H, W, Cout, ks, lstm_hid); stride 1, "same" padding
_C3 = [
    # BM = 32
    (2, [40], 8, 8, 24, 3, 0), (4, [64], 7, 7, 32, 3, 0), (2, [24, 8], 16, 16, 32, 3, 8), (2, [8], 9, 11, 16, 3, 0),
    (2, [16], 16, 32, 24, 3, 0), (2, [20, 12], 17, 23, 24, 3, 0),
    # BM = 64
    (2, [72], 8, 8, 72, 3, 0), (4, [64], 7, 7, 256, 3, 0), (2, [72], 5, 13, 200, 3, 0), (2, [72], 8, 16, 200, 3, 0),
    (2, [200], 8, 32, 136, 3, 0), (2, [40], 17, 23, 72, 3, 0), (3, [64], 14, 14, 64, 3, 0), (2, [200], 7, 7, 72, 3, 0),
    # BM = 128 (Cout > 64 and Cs > 512)
    (1, [520], 8, 8, 72, 3, 0), (1, [520], 7, 7, 72, 3, 0), (1, [520], 4, 16, 136, 3, 0), (1, [544], 14, 14, 72, 3, 0),
    (1, [520], 2, 32, 72, 3, 0), (1, [520], 3, 18, 72, 3, 0),
    # 1 / 2 / 3 spatial tiles per block
    (1, [32], 4, 16, 64, 3, 0), (2, [32], 4, 16, 64, 3, 0), (3, [32], 4, 16, 64, 3, 0),
    # the gate conv of the step, gate-interleaved dy rows, two sources
    (2, [128, 64], 16, 16, 256, 3, 64),
]
_C1 = [
    (2, [64], 8, 32, 64, 1, 0), (3, [40], 7, 7, 48, 1, 0), (2, [256], 16, 16, 64, 1, 0), (3, [96], 7, 7, 48, 1, 0),
    (2, [64], 16, 16, 256, 1, 0), (2, [40], 9, 11, 136, 1, 0), (1, [16], 30, 27, 96, 1, 0), (2, [136], 16, 16, 264, 1, 0),
    (2, [200], 16, 16, 72, 1, 0), (1, [136], 5, 13, 200, 1, 0), (1, [32], 4, 16, 64, 1, 0), (3, [32], 4, 16, 64, 1, 0),
]
# the shapes that hold the time of the 256 x 256 training step (tests/test_gpu_wgrad_limbs.py _STEP), B = 4
_STEP = [(4, [256], 16, 16, 256, 3, 0), (4, [1024], 16, 16, 256, 1, 0), (4, [256], 16, 16, 1024, 1, 0), (4, [128, 64], 16, 16, 256, 3, 64)]
# kind: "" plain, "hot" per-pixel powers of two (|dy * x| from 2^-20 to 2^20 inside one reduction), "inf" one +inf in x
CASES = [c + ("",) for c in _C3 + _C1 + _STEP] + [(2, [64], 16, 16, 64, 3, 0, "hot"), (2, [64], 16, 16, 64, 3, 0, "inf"),
                                                 (2, [64], 16, 16, 64, 1, 0, "inf")]
INF_AT = (1, 5, 7, 9)        # (image, channel, y, x): an interior pixel, so every tap of a 3x3 sees it
# more jobs than one grouped launch holds, all of one instantiation (their own grouped call)
MANY = [(1, [32], 8, 8, 32, 3, 0, "")] * (WGB_MAXJ + 8)


def _instantiation(c):
    B, segs, H, W, Cout, ks = c[:6]
    out = set()
    for Cs in segs:
        if ks == 3:
            out.add((3, 32 if Cout <= 32 else (64 if (Cout <= 64 or Cs <= 512) else 128), 32 if W > 16 else (16 if W > 8 else 8), W % 4 == 0))
        else:
            out.add((1, 64 if Cout <= 64 else 128, 64 if Cs <= 64 else 128, (H * W) % 4 == 0))
    return out


def test_every_instantiation_has_a_case():
    have = set().union(*[_instantiation(c) for c in CASES])
    want = ({(3, bm, tw, v4) for bm in (32, 64, 128) for tw in (8, 16, 32) for v4 in (False, True)}
            | {(1, bm, bn, v4) for bm in (64, 128) for bn in (64, 128) for v4 in (False, True)})
    assert want <= have, "no case for %r" % sorted(want - have)


def _rng_t(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, 1.0, shape).astype(np.float32))


def _inputs(cases, k, base=0):
    B, segs, H, W, Cout, ks, hid, kind = cases[k]
    xs = [_rng_t(base + 17000 + 10 * k + i, (B, c, H, W)) for i, c in enumerate(segs)]
    gy = _rng_t(base + 19000 + k, (B, Cout, H, W))
    if kind == "hot":
        r = np.random.default_rng(16000 + k)
        gy = gy * torch.from_numpy(np.exp2(r.integers(-10, 11, (B, 1, H, W))).astype(np.float32))
        xs = [x * torch.from_numpy(np.exp2(r.integers(-10, 11, (B, 1, H, W))).astype(np.float32)) for x in xs]
    if kind == "inf":
        xs[0][INF_AT] = float("inf")
    prev = _rng_t(base + 20000 + k, (Cout, sum(segs), ks, ks))
    return xs, gy, prev


def _reference(cases, k, base=0):
    B, segs, H, W, Cout, ks, hid, kind = cases[k]
    xs, gy, prev = _inputs(cases, k, base)
    x = torch.cat(xs, 1).double()
    if kind == "inf":        # the reduction that contains the inf is marked below (_inf_mask); the reference of the rest is the finite sum
        x[INF_AT] = 0.0
    wd = torch.zeros(Cout, sum(segs), ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wd, None, stride=1, padding=ks // 2).backward(gy.double())
    return prev.double() + wd.grad


def _inf_mask(c):
    """dW elements whose reduction contains the +inf: every output row and tap of the inf's input channel (an interior pixel)"""
    B, segs, H, W, Cout, ks, hid, kind = c
    m = torch.zeros(Cout, sum(segs), ks, ks, dtype=torch.bool)
    if kind == "inf":
        m[:, INF_AT[1]] = True
    return m


def _run(cases, grouped, base=0):
    """dW of every case (on top of its pre-filled contents) through rsis_conv2d_wgrad / one rsis_conv2d_wgrad_batch call"""
    from rsis_amd import ops
    from rsis_amd._lib import WgradJob, check, lib, ptr, stream
    L = lib()
    jobs, keep, out = [], [], []
    for k, (B, segs, H, W, Cout, ks, hid, kind) in enumerate(cases):
        Ctot, pad = sum(segs), ks // 2
        xs, gy, prev = _inputs(cases, k, base)
        if hid > 0:       # the kernel sees gate-interleaved dy rows 4 j + g and writes reference row g * hid + j
            gy = gy.reshape(B, 4, hid, H, W).transpose(1, 2).reshape(B, Cout, H, W).contiguous()
        dW, dy = prev.clone().cuda(), gy.cuda()
        c_off = 0
        for x in xs:
            xd = x.cuda()
            if grouped:
                j = WgradJob()
                (j.dy, j.x, j.dW, j.B, j.Cs, j.H, j.W, j.Cout, j.Ho, j.Wo, j.ks, j.stride, j.pad, j.Ctot, j.c_off, j.lstm_hid, j.dtype) = (
                    dy.data_ptr(), xd.data_ptr(), dW.data_ptr(), B, x.shape[1], H, W, Cout, H, W, ks, 1, pad, Ctot, c_off, hid, ops.DTYPE_F32)
                jobs.append(j)
            else:
                check(L.rsis_conv2d_wgrad(ptr(dy), ptr(xd), ptr(dW), B, x.shape[1], H, W, Cout, H, W, ks, 1, pad, Ctot, c_off, hid,
                                          ops.DTYPE_F32, stream()), "rsis_conv2d_wgrad")
            keep.append(xd)
            c_off += x.shape[1]
        keep.append(dy)
        out.append(dW)
    if grouped:
        arr = (WgradJob * len(jobs))(*jobs)
        check(L.rsis_conv2d_wgrad_batch(arr, len(jobs), stream()), "rsis_conv2d_wgrad_batch")
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _refused():
    """return codes of two jobs the staged kernels do not take: a stride-2 3x3 and a Cout == 1 conv, single and as a batch of one"""
    from rsis_amd import ops
    from rsis_amd._lib import WgradJob, lib, ptr, stream
    L = lib()
    codes = []
    for (B, Cs, H, W, Cout, ks, stride, pad) in ((2, 24, 32, 48, 40, 3, 2, 1), (2, 16, 16, 16, 1, 3, 1, 1)):
        Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        x, dy, dW = torch.zeros(B, Cs, H, W).cuda(), torch.zeros(B, Cout, Ho, Wo).cuda(), torch.zeros(Cout, Cs, ks, ks).cuda()
        codes.append(int(L.rsis_conv2d_wgrad(ptr(dy), ptr(x), ptr(dW), B, Cs, H, W, Cout, Ho, Wo, ks, stride, pad, Cs, 0, 0, ops.DTYPE_F32, stream())))
        j = WgradJob()
        (j.dy, j.x, j.dW, j.B, j.Cs, j.H, j.W, j.Cout, j.Ho, j.Wo, j.ks, j.stride, j.pad, j.Ctot, j.c_off, j.lstm_hid, j.dtype) = (
            dy.data_ptr(), x.data_ptr(), dW.data_ptr(), B, Cs, H, W, Cout, Ho, Wo, ks, stride, pad, Cs, 0, 0, ops.DTYPE_F32)
        codes.append(int(L.rsis_conv2d_wgrad_batch((WgradJob * 1)(j), 1, stream())))
        torch.cuda.synchronize()
    return codes


def _run_all():
    from rsis_amd import ops
    res = {"single": _run(CASES, False), "grouped": _run(CASES, True), "many": _run(MANY, True, base=500000), "refused": _refused()}
    prev = ops.set_deterministic(True)
    try:
        for name, grouped in (("single", False), ("grouped", True)):
            res["det_a_" + name] = _run(CASES, grouped)
            res["det_b_" + name] = _run(CASES, grouped)
    finally:
        ops.set_deterministic(prev)
    return res


def _child(mode, path):
    env = dict(os.environ, RSIS_WGRAD_LIMBS=mode)
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path], env=env, check=True)
    return torch.load(path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wgrad_staged")
    out = {"ref": [_reference(CASES, k) for k in range(len(CASES))], "ref_many": [_reference(MANY, k, 500000) for k in range(len(MANY))]}
    for name, mode in (("f32", "0"), ("reg_all", "all"), ("staged", "staged"), ("reg", "reg")):      # (check=True: a failed child ends the chain)
        out[name] = _child(mode, str(d / (name + ".pt")))
    out["table"] = _run_all()
    return out


def _err(got, ref, cases):
    """max |got - ref| over the elements whose reduction holds no inf"""
    return [float((g.double() - r)[~_inf_mask(c)].abs().max()) for g, r, c in zip(got, ref, cases)]


def _bars(runs, key, refkey, cases, which):
    ref = runs[refkey]
    e32, ereg, el = _err(runs["f32"][key], ref, cases), _err(runs["reg_all"][key], ref, cases), _err(runs[which][key], ref, cases)
    bad = []
    for k, c in enumerate(cases):
        bar = 2e-5 * max(1.0, float(ref[k].abs().max()))
        print("case %2d %-58r e32 %.3e  e_reg %.3e  %s %.3e  ratio %.2f  bar %.3e" % (k, c, e32[k], ereg[k], which, el[k],
                                                                                     el[k] / max(e32[k], ereg[k], 1e-300), bar))
        if not (el[k] <= 2.0 * max(e32[k], ereg[k]) and el[k] <= bar):
            bad.append((k, c, e32[k], ereg[k], el[k], bar))
    assert not bad, "beyond 2 x max(e32, e_reg) or beyond 2e-5 * max(1, max |ref|): %r" % bad


@pytest.mark.parametrize("which", ["staged", "table"], ids=["every-job-staged", "default-table"])
@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_staged_limbs_against_float64_the_f32_loop_and_the_register_split_loop(runs, mode, which):
    _bars(runs, mode, "ref", CASES, which)


@pytest.mark.parametrize("which", ["staged", "table"], ids=["every-job-staged", "default-table"])
def test_grouped_call_of_more_jobs_than_one_launch_holds(runs, which):
    _bars(runs, "many", "ref_many", MANY, which)


@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_one_inf_reaches_exactly_the_reductions_that_contain_it(runs, mode):
    n = 0
    for k, c in enumerate(CASES):
        if c[7] != "inf":
            continue
        n += 1
        for which in ("f32", "staged"):
            got = runs[which][mode][k]
            assert torch.equal(~torch.isfinite(got), _inf_mask(c)), "case %d %r (%s): non-finite dW elements are not the inf's reductions" % (k, c, which)
    assert n == 2


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_staged_is_deterministic_in_deterministic_mode(runs, mode):
    for k, (a, b) in enumerate(zip(runs["staged"]["det_a_" + mode], runs["staged"]["det_b_" + mode])):
        assert torch.equal(_bits(a), _bits(b)), "case %d %r: two deterministic calls differ" % (k, CASES[k])
    el = _err(runs["staged"]["det_a_" + mode], runs["ref"], CASES)
    for k in range(len(CASES)):
        assert el[k] <= 2e-5 * max(1.0, float(runs["ref"][k].abs().max())), (k, CASES[k], el[k])


@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_deterministic_mode_does_not_reroute(runs, mode):
    for k, (a, b) in enumerate(zip(runs["table"]["det_a_" + mode], runs["reg"]["det_a_" + mode])):
        assert torch.equal(_bits(a), _bits(b)), "case %d %r: the default and RSIS_WGRAD_LIMBS=reg differ in deterministic mode" % (k, CASES[k])


PARENT_DUMP = os.path.join(ROOT, "gpu_jobs", "wgrad_staged_parent_dw.pt")


@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_staged_reproduces_the_parent_build(runs, mode):
    """RSIS_WGRAD_LIMBS=staged in deterministic mode against the bits of the parent build (one contributor per dW element, so the
    bits are a function of the kernel alone).  The dump is a measurement the parent build writes with this file as a script
    (`RSIS_WGRAD_LIMBS=staged RSIS_HIP_LIB=<parent library> python tests/test_gpu_wgrad_staged.py gpu_jobs/wgrad_staged_parent_dw.pt dump`),
    not a golden."""
    if not os.path.exists(PARENT_DUMP):
        pytest.skip("no dump of the parent build's dW at gpu_jobs/wgrad_staged_parent_dw.pt")
    parent = torch.load(PARENT_DUMP)
    assert len(parent[mode]) == len(CASES)
    for k, (a, b) in enumerate(zip(runs["staged"]["det_a_" + mode], parent[mode])):
        assert torch.equal(_bits(a), _bits(b)), "case %d %r: RSIS_WGRAD_LIMBS=staged differs from the parent build" % (k, CASES[k])


def _dump():
    """the deterministic-mode dW of CASES, single and grouped (written under RSIS_WGRAD_LIMBS=staged by the parent build)"""
    from rsis_amd import ops
    assert os.environ.get("RSIS_WGRAD_LIMBS") == "staged", "the dump is of the staged kernels: run under RSIS_WGRAD_LIMBS=staged"
    prev = ops.set_deterministic(True)
    try:
        return {"single": _run(CASES, False), "grouped": _run(CASES, True)}
    finally:
        ops.set_deterministic(prev)


def test_staged_refuses_what_its_kernels_do_not_take(runs):
    assert runs["staged"]["refused"] == [ERR_UNSUPPORTED] * 4, runs["staged"]["refused"]
    assert runs["reg"]["refused"] == [0] * 4 and runs["table"]["refused"] == [0] * 4      # (the other modes route them as before)


if __name__ == "__main__":
    torch.save(_dump() if sys.argv[2:] == ["dump"] else _run_all(), sys.argv[1])
