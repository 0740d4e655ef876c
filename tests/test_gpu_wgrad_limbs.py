"""fp32 weight gradients on the split-bf16 MFMA (the LIMB loop of rsis_amd/csrc/conv_wgrad_tiled.hip: three exact bf16 limbs per operand,
six limb products per K16 step) against FLOAT64 autograd of F.conv2d (nn.Conv2d of reference src/modules/clstm.py:17,44), next to the
exact-f32 loop on the same inputs.  Bars, stated before the kernel ran:

  * on every case the limb loop is no further from float64 than 2 x the f32 loop's own error e32 (the rule tests/test_gpu_wino.py
    applies to a changed arithmetic), and inside the bar of test_conv2d_wgrad_fp32_on_ragged_maps, 2e-5 * max(1, max |ref|);
  * the same on a hot case whose products |dy * x| span 2^-20 .. 2^20 inside one reduction;
  * deterministic mode: two calls give equal bits;
  * RSIS_WGRAD_LIMBS=0 reproduces the parent build's bits (against a dump the parent build wrote; skipped when there is none).

RSIS_WGRAD_LIMBS is read once per process, so the f32 loop (=0) and the limb loop on EVERY tile configuration (=all) run in child
processes (this file, as a script); the default (the measured per-configuration table) runs in the test process.  The cases: the
shapes of RAGGED_WGRAD_CASES and of test_conv2d_wgrad_batch (tests/test_gpu_ops.py), restated, plus the four shapes that hold the
time of a training step.  Every case runs as single launches and in one grouped call, each on top of a pre-filled dW."""
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

# (B, [Cin segs], H, W, Cout, ks, stride, pad, lstm_hid, hot)
_RAGGED = [(3, [64], 14, 14, 64, 3, 0), (2, [128], 28, 28, 128, 3, 0), (4, [64], 7, 7, 256, 3, 0), (2, [256], 14, 14, 1024, 1, 0),
           (2, [1024], 14, 14, 256, 1, 0), (3, [96], 7, 7, 48, 1, 0), (2, [8], 9, 11, 16, 3, 0), (2, [20, 12], 17, 23, 40, 3, 0),
           (2, [72], 5, 13, 200, 3, 0), (3, [40], 12, 18, 24, 1, 0), (2, [24, 8], 14, 14, 32, 3, 8), (1, [16], 30, 27, 96, 1, 0),
           (2, [16], 28, 28, 32, 3, 0), (2, [200], 7, 7, 72, 3, 0)]
_BATCH = [(2, [16], 16, 16, 32, 3, 1, 1, 0), (2, [16], 16, 32, 64, 3, 1, 1, 0), (2, [32], 16, 16, 128, 3, 1, 1, 0),
          (2, [64], 8, 32, 96, 1, 1, 0, 0), (2, [20, 12], 16, 24, 40, 3, 1, 1, 0), (2, [72], 8, 16, 200, 3, 1, 1, 0),
          (3, [40], 12, 16, 24, 1, 1, 0, 0), (2, [24, 8], 16, 16, 32, 3, 1, 1, 8), (2, [8], 9, 11, 16, 3, 1, 1, 0),
          (2, [24], 32, 48, 40, 3, 2, 1, 0), (2, [256], 16, 16, 256, 3, 1, 1, 0), (2, [256], 16, 16, 64, 1, 1, 0, 0),
          (2, [64], 16, 16, 256, 1, 1, 0, 0), (1, [256], 16, 16, 256, 3, 1, 1, 0)]
# the shapes that hold the time of the 256 x 256 training step: layer-3 3x3, the bottleneck 1x1 pair, a ConvLSTM gate conv (two sources)
_STEP = [(4, [256], 16, 16, 256, 3, 1, 1, 0), (4, [1024], 16, 16, 256, 1, 1, 0, 0), (4, [256], 16, 16, 1024, 1, 1, 0, 0),
         (2, [128, 64], 16, 16, 256, 3, 1, 1, 64)]
CASES = ([(B, s, H, W, Co, ks, 1, ks // 2, hid, False) for (B, s, H, W, Co, ks, hid) in _RAGGED] + [c + (False,) for c in _BATCH]
         + [c + (False,) for c in _STEP] + [(2, [64], 16, 16, 64, 3, 1, 1, 0, True)])


def _rng_t(seed, shape, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32))


def _inputs(k):
    B, segs, H, W, Cout, ks, stride, pad, hid, hot = CASES[k]
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    xs = [_rng_t(7000 + 10 * k + i, (B, c, H, W)) for i, c in enumerate(segs)]
    gy = _rng_t(9000 + k, (B, Cout, Ho, Wo))
    if hot:      # per-pixel powers of two: |dy * x| spans 2^-20 .. 2^20 along the reduction (the pixels) of every dW element
        r = np.random.default_rng(6000 + k)
        gy = gy * torch.from_numpy(np.exp2(r.integers(-10, 11, (B, 1, Ho, Wo))).astype(np.float32))
        xs = [x * torch.from_numpy(np.exp2(r.integers(-10, 11, (B, 1, H, W))).astype(np.float32)) for x in xs]
    prev = _rng_t(10000 + k, (Cout, sum(segs), ks, ks))
    return xs, gy, prev


def _reference(k):
    B, segs, H, W, Cout, ks, stride, pad, hid, hot = CASES[k]
    xs, gy, prev = _inputs(k)
    wd = torch.zeros(Cout, sum(segs), ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(torch.cat(xs, 1).double(), wd, None, stride=stride, padding=pad).backward(gy.double())
    return prev.double() + wd.grad


def _run(grouped):
    """dW of every case (on top of its pre-filled contents) through rsis_conv2d_wgrad / one rsis_conv2d_wgrad_batch call"""
    from rsis_amd import ops
    from rsis_amd._lib import WgradJob, check, lib, ptr, stream
    L = lib()
    jobs, keep, out = [], [], []
    for k, (B, segs, H, W, Cout, ks, stride, pad, hid, hot) in enumerate(CASES):
        Ctot = sum(segs)
        Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        xs, gy, prev = _inputs(k)
        if hid > 0:       # the kernel sees gate-interleaved dy rows 4 j + g and writes reference row g * hid + j
            gy = gy.reshape(B, 4, hid, Ho, Wo).transpose(1, 2).reshape(B, Cout, Ho, Wo).contiguous()
        dW, dy = prev.clone().cuda(), gy.cuda()
        c_off = 0
        for x in xs:
            xd = x.cuda()
            if grouped:
                j = WgradJob()
                (j.dy, j.x, j.dW, j.B, j.Cs, j.H, j.W, j.Cout, j.Ho, j.Wo, j.ks, j.stride, j.pad, j.Ctot, j.c_off, j.lstm_hid, j.dtype) = (
                    dy.data_ptr(), xd.data_ptr(), dW.data_ptr(), B, x.shape[1], H, W, Cout, Ho, Wo, ks, stride, pad, Ctot, c_off, hid, ops.DTYPE_F32)
                jobs.append(j)
            else:
                check(L.rsis_conv2d_wgrad(ptr(dy), ptr(xd), ptr(dW), B, x.shape[1], H, W, Cout, Ho, Wo, ks, stride, pad, Ctot, c_off, hid,
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


def _run_all():
    from rsis_amd import ops
    res = {"single": _run(False), "grouped": _run(True)}
    prev = ops.set_deterministic(True)
    try:
        for name, grouped in (("single", False), ("grouped", True)):
            res["det_a_" + name] = _run(grouped)
            res["det_b_" + name] = _run(grouped)
    finally:
        ops.set_deterministic(prev)
    return res


def _child(mode, path, lib=None):
    env = dict(os.environ, RSIS_WGRAD_LIMBS=mode)
    if lib:
        env["RSIS_HIP_LIB"] = lib
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, timeout=600)
    return torch.load(path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wgrad_limbs")
    ref = [_reference(k) for k in range(len(CASES))]
    return {"ref": ref, "f32": _child("0", str(d / "f32.pt")), "limb": _child("all", str(d / "limb.pt")), "table": _run_all()}


def _err(got, ref):
    return [float((g.double() - r).abs().max()) for g, r in zip(got, ref)]


@pytest.mark.parametrize("which", ["limb", "table"], ids=["every-configuration", "default-table"])
@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_limb_loop_against_float64_and_the_f32_loop(runs, mode, which):
    ref = runs["ref"]
    e32, el = _err(runs["f32"][mode], ref), _err(runs[which][mode], ref)
    bad = []
    for k, c in enumerate(CASES):
        bar = 2e-5 * max(1.0, float(ref[k].abs().max()))
        print("case %2d %-52r e32 %.3e  limb %.3e  ratio %.2f  bar %.3e" % (k, c, e32[k], el[k], el[k] / max(e32[k], 1e-300), bar))
        if not (el[k] <= 2.0 * e32[k] and el[k] <= bar):
            bad.append((k, c, e32[k], el[k], bar))
    assert not bad, "limb loop beyond 2 x e32 or beyond 2e-5 * max(1, max |ref|): %r" % bad


@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_limb_loop_is_deterministic_in_deterministic_mode(runs, mode):
    for which in ("limb", "table"):
        for k, (a, b) in enumerate(zip(runs[which]["det_a_" + mode], runs[which]["det_b_" + mode])):
            assert torch.equal(a, b), "case %d %r (%s): two deterministic calls differ" % (k, CASES[k], which)
        el = _err(runs[which]["det_a_" + mode], runs["ref"])
        for k in range(len(CASES)):
            assert el[k] <= 2e-5 * max(1.0, float(runs["ref"][k].abs().max())), (k, CASES[k], el[k])


PARENT_DUMP = os.path.join(ROOT, "gpu_jobs", "wgrad_limbs_parent_dw.pt")


@pytest.mark.parametrize("mode", ["single", "grouped"])
def test_knob_off_reproduces_the_parent_build(runs, mode):
    """RSIS_WGRAD_LIMBS=0 against the bits of the parent build (deterministic mode: one contributor per dW element, so the bits are
    a function of the kernel alone).  The dump is a measurement the parent build writes with this file as a script
    (`RSIS_HIP_LIB=<parent library> python tests/test_gpu_wgrad_limbs.py gpu_jobs/wgrad_limbs_parent_dw.pt`), not a golden."""
    if not os.path.exists(PARENT_DUMP):
        pytest.skip("no dump of the parent build's dW at gpu_jobs/wgrad_limbs_parent_dw.pt")
    parent = torch.load(PARENT_DUMP)
    for k, (a, b) in enumerate(zip(runs["f32"]["det_a_" + mode], parent["det_a_" + mode])):
        assert torch.equal(a, b), "case %d %r: RSIS_WGRAD_LIMBS=0 differs from the parent build" % (k, CASES[k])


if __name__ == "__main__":
    torch.save(_run_all(), sys.argv[1])
