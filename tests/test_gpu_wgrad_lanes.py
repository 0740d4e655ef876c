"""The grouped XCD-lane launch of the bf16 weight gradients -- what every bf16 training step runs (ops.flush_wgrads: ~40 layers in one
rsis_conv2d_wgrad_batch call) -- against FLOAT64, for the register-staged kernels (RSIS_DTYPE_BF16: wgrad3_bf16_group_kernel /
wgrad1_bf16_group_kernel, 18 + 8 instantiations) and the blk DMA kernels (RSIS_DTYPE_BF16_BLK: wgrad3_tr_group_kernel /
wgrad1_tr_group_kernel, 9 + 4 instantiations).  Cases, reference and the two bars (TIGHT, ROUNDING) are tests/wgrad_lane_cases.py;
tests/test_wgrad_lane_bars_host.py shows that the bars reject a dropped tile, a doubled split, transposed taps and truncation.

Why this file runs in DEFAULT mode: rsis_conv2d_wgrad_batch (csrc/api.hip) groups a job only under
`(route == 1 || route == 2) && (q.ks == 1 || q.ks == 3) && !rsis_deterministic()` ("grouped below"); in deterministic mode it launches
every job on its own, in the plain mode of wgb_find.  So only with the deterministic mode off does a batch call reach
wgb_plan_lanes and the lane branch of wgb_find.

  * default mode, this process: every call of wgrad_lane_cases.CALLS as single launches (rsis_conv2d_wgrad: plain mode) and as ONE
    rsis_conv2d_wgrad_batch call (lane mode), TIGHT on both; one +inf in x makes exactly its own reductions non-finite;
  * RSIS_WGB_GROUP_BLOCKS=8 (read once per process: a child, this file as a script): a bucket's blocks walk total / 8 spatial tiles
    each, the rings of depth 2-3 wrap, jobs get 1-8 splits.  Grouped calls only, ROUNDING; err / TIGHT is printed (and written next
    to the margins when RSIS_TEST_MARGINS is set), not asserted;
  * the canary: the knob does nothing in plain mode, so per family at least one case with more than two spatial tiles must differ in
    bits between the default grouped run and the knob run; and every case that the knob cuts into one split per job (lane_splits of
    wgrad_lane_cases.py, the planner's rule restated) has exactly the deterministic mode's bits in the knob run, while the default run,
    cut at L = 2, does not;
  * deterministic mode: two grouped calls (one plain-mode launch per job) give equal bits and satisfy ROUNDING;
  * a blk job with Cs = 12 and a blk stride-2 job, each as a batch of one, return RSIS_ERR_UNSUPPORTED and leave dW untouched.
No case is skipped or filtered."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import wgrad_lane_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 3
SENTINEL = -12345.5


def _blk(t):
    """NCHW fp32 -> channel-blocked bf16 [B][C / 8][H][W][8]"""
    B, C, H, W = t.shape
    return t.reshape(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)


def _job(c, j, dy, x, dW):
    from rsis_amd import ops
    from rsis_amd._lib import WgradJob
    q = WgradJob()
    dtype = {"f32": ops.DTYPE_F32, "bf16": ops.DTYPE_BF16, "blk": ops.DTYPE_BF16_BLK}[c.dtype]
    (q.dy, q.x, q.dW, q.B, q.Cs, q.H, q.W, q.Cout, q.Ho, q.Wo, q.ks, q.stride, q.pad, q.Ctot, q.c_off, q.lstm_hid, q.dtype) = (
        dy[j.img0:].data_ptr(), x.data_ptr(), dW.data_ptr(), j.B, j.Cs, c.H, c.W, c.Cout, c.Ho, c.Wo, c.ks, c.stride, c.pad, c.Ctot, j.c_off,
        c.hid, dtype)
    return q


def _run(grouped):
    """dW of every case of every call, on top of its pre-filled contents: {call: [dW, ...]}.  grouped: ONE rsis_conv2d_wgrad_batch per
    call (the mixed call's jobs in MIXED_ORDER); else job by job through rsis_conv2d_wgrad"""
    from rsis_amd._lib import WgradJob, check, lib, stream
    L = lib()
    out = {}
    for call, cases in LC.CALLS.items():
        jobs, keep, dWs = [], [], []
        for c in cases:
            dys, xs, prev = LC.inputs(c)
            if c.hid > 0:       # the kernel sees gate-interleaved dy rows 4 j + g and writes reference row g * hid + j
                dys = [d.reshape(d.shape[0], 4, c.hid, c.Ho, c.Wo).transpose(1, 2).reshape(d.shape[0], c.Cout, c.Ho, c.Wo).contiguous() for d in dys]
            up = (lambda t: _blk(t).cuda()) if c.dtype == "blk" else (lambda t: t.cuda())
            dyd, xd, dW = [up(d) for d in dys], [up(x) for x in xs], prev.clone().cuda()
            keep += dyd + xd
            dWs.append(dW)
            jobs += [_job(c, j, dyd[j.dy], x, dW) for j, x in zip(c.jobs, xd)]
        if call == "mixed":
            jobs = [jobs[i] for i in LC.MIXED_ORDER]
        if grouped:
            check(L.rsis_conv2d_wgrad_batch((WgradJob * len(jobs))(*jobs), len(jobs), stream()), "rsis_conv2d_wgrad_batch(%s)" % call)
        else:
            for q in jobs:
                check(L.rsis_conv2d_wgrad(q.dy, q.x, q.dW, q.B, q.Cs, q.H, q.W, q.Cout, q.Ho, q.Wo, q.ks, q.stride, q.pad, q.Ctot, q.c_off,
                                          q.lstm_hid, q.dtype, stream()), "rsis_conv2d_wgrad(%s)" % call)
        torch.cuda.synchronize()
        out[call] = [t.cpu() for t in dWs]
    return out


def _refused():
    """[(return code, dW untouched)] of a blk job with Cs = 12 and a blk stride-2 job, each as a batch of one"""
    from rsis_amd import ops
    from rsis_amd._lib import WgradJob, lib, stream
    res = []
    for (B, Cs, H, W, Cout, stride) in ((2, 12, 8, 8, 16, 1), (2, 16, 16, 16, 16, 2)):
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        x = torch.zeros(B, (Cs + 7) // 8, H, W, 8, dtype=torch.bfloat16).cuda()
        dy = torch.zeros(B, Cout // 8, Ho, Wo, 8, dtype=torch.bfloat16).cuda()
        dW = torch.full((Cout, Cs, 3, 3), SENTINEL).cuda()
        q = WgradJob()
        (q.dy, q.x, q.dW, q.B, q.Cs, q.H, q.W, q.Cout, q.Ho, q.Wo, q.ks, q.stride, q.pad, q.Ctot, q.c_off, q.lstm_hid, q.dtype) = (
            dy.data_ptr(), x.data_ptr(), dW.data_ptr(), B, Cs, H, W, Cout, Ho, Wo, 3, stride, 1, Cs, 0, 0, ops.DTYPE_BF16_BLK)
        rc = int(lib().rsis_conv2d_wgrad_batch((WgradJob * 1)(q), 1, stream()))
        torch.cuda.synchronize()
        res.append((rc, bool((dW == SENTINEL).all())))
    return res


def _child(path):
    env = dict(os.environ, RSIS_WGB_GROUP_BLOCKS="8")
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path], env=env, check=True)
    return torch.load(path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from rsis_amd import ops
    for c in LC.ALL_CASES:
        LC.reference(c)
    prev = ops.set_deterministic(False)       # (whatever RSIS_DETERMINISTIC says: the default runs are the lane mode)
    try:
        out = {"single": _run(False), "grouped": _run(True), "refused": _refused()}
        ops.set_deterministic(True)
        out["det_a"], out["det_b"] = _run(True), _run(True)
    finally:
        ops.set_deterministic(prev)
    out["knob"] = _child(str(tmp_path_factory.mktemp("wgrad_lanes") / "knob.pt"))
    return out


def _unasserted(tag, call, c, r):
    print("%-12s %-28s err / TIGHT %.4f" % (tag, c.name, r))
    if os.environ.get("RSIS_TEST_MARGINS"):
        with open(os.environ["RSIS_TEST_MARGINS"] + ".unasserted", "a") as f:
            f.write("%.4f\t%s\t%s\t%s\terr / TIGHT, not asserted\n" % (r, tag, call, c.name))


@pytest.mark.parametrize("call", list(LC.CALLS))
@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_default_mode_meets_tight(runs, mode, call):
    for c, got in zip(LC.CALLS[call], runs[mode][call]):
        assert torch.equal(~torch.isfinite(got), LC.reference(c)["mask"]), "%r (%s): the non-finite dW elements are not the inf's reductions" % (c, mode)
        LC.check(mode, c, got, "TIGHT")


@pytest.mark.parametrize("call", list(LC.CALLS))
def test_knob_run_meets_rounding(runs, call):
    for c, got in zip(LC.CALLS[call], runs["knob"][call]):
        assert torch.equal(~torch.isfinite(got), LC.reference(c)["mask"]), "%r: the non-finite dW elements are not the inf's reductions" % (c,)
        _unasserted("knob", call, c, LC.ratio(c, got, "TIGHT")[0])
        LC.check("RSIS_WGB_GROUP_BLOCKS=8 grouped", c, got, "ROUNDING")


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_the_grouped_call_was_grouped(runs, family):
    """the knob only changes the plan of wgb_plan_lanes: where no case with more than two spatial tiles changes its bits, the batch call
    did not run in lane mode"""
    differ, seen = 0, 0
    for call, cases in LC.CALLS.items():
        if LC.family_of(call) != family:
            continue
        for c, a, b in zip(cases, runs["grouped"][call], runs["knob"][call]):
            if c.kind != "inf" and max(LC.spatial_tiles(c, j) for j in c.jobs) > 2:
                seen += 1
                differ += not torch.equal(a.view(torch.int32), b.view(torch.int32))
    print("%s: %d of %d cases with more than two spatial tiles differ between the default and the knob run" % (family, differ, seen))
    one, knob_eq, dflt_eq = 0, 0, 0
    for call, cases in LC.CALLS.items():
        if LC.family_of(call) != family:
            continue
        at8, at896 = LC.lane_splits(call, 8), LC.lane_splits(call, LC.WGB_TARGET)
        for c, a, b, d in zip(cases, runs["grouped"][call], runs["knob"][call], runs["det_a"][call]):
            if c.kind != "inf" and max(at8[c.name]) == 1 and min(at896[c.name]) > 1 and float(LC.reference(c)["k"].max()) == 1:
                one += 1
                knob_eq += torch.equal(b.view(torch.int32), d.view(torch.int32))
                dflt_eq += torch.equal(a.view(torch.int32), d.view(torch.int32))
    print("%s: of %d cases cut into one split per job by the knob and into more by default, %d knob runs and %d default runs have the "
          "deterministic mode's bits" % (family, one, knob_eq, dflt_eq))
    # (two grouped runs can also differ by the order of their atomics alone.  This cannot: a job cut into ONE split has one contributor
    #  per dW element, which walks the job's tiles in the deterministic mode's order -- the knob run of such a case has exactly the
    #  deterministic mode's bits, and the default run, cut at L = 2, has other partial sums)
    assert one > 0 and knob_eq == one, "%s: %d of %d one-split knob runs differ from the deterministic mode's bits" % (family, one - knob_eq, one)
    assert dflt_eq < one, "%s: the grouped call was not grouped: every default run has the bits of one split per job" % family
    assert seen > 0
    assert differ > 0, "%s: the grouped call was not grouped: RSIS_WGB_GROUP_BLOCKS=8 changed no bit of any of %d cases" % (family, seen)


@pytest.mark.parametrize("call", list(LC.CALLS))
def test_deterministic_mode_is_deterministic_and_meets_rounding(runs, call):
    for c, a, b in zip(LC.CALLS[call], runs["det_a"][call], runs["det_b"][call]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%r: two deterministic grouped calls differ" % (c,)
        assert torch.equal(~torch.isfinite(a), LC.reference(c)["mask"])
        _unasserted("det", call, c, LC.ratio(c, a, "TIGHT")[0])
        LC.check("deterministic grouped", c, a, "ROUNDING")


def test_blk_refuses_what_its_kernels_do_not_take(runs):
    assert runs["refused"] == [(ERR_UNSUPPORTED, True)] * 2, runs["refused"]


if __name__ == "__main__":
    from rsis_amd import ops
    ops.set_deterministic(False)
    torch.save(_run(True), sys.argv[1])
