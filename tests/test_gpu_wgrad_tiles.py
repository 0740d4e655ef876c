"""Grouped fp32 weight gradients (rsis_amd/csrc/conv_wgrad_tiled.hip) on the wider tiles a grouped launch may take (RSIS_WGRAD_TILES)
and in the XCD-contiguous block order (RSIS_WGRAD_XCD), against FLOAT64 autograd of F.conv2d (nn.Conv2d of reference
src/modules/clstm.py:17,44).  The structure and the bars are those of tests/test_gpu_wgrad_limbs.py, stated before the kernels ran:

  * under RSIS_WGRAD_TILES=wide, on the f32 loop (RSIS_WGRAD_LIMBS=0) and on the limb loop (=all), every case is no further from
    float64 than 2 x the error e32 of the single launch's tile rule on the f32 loop (RSIS_WGRAD_TILES=0 RSIS_WGRAD_LIMBS=0) on the
    same case, and inside 2e-5 * max(1, max |ref|);
  * deterministic mode: two calls give equal bits, and RSIS_WGRAD_XCD=0 (hardware order everywhere) gives the bits of the default
    (the measured per-bucket table) and of RSIS_WGRAD_XCD=all (XCD-contiguous order everywhere): one contributor per dW tile, so
    the block order cannot show;
  * otherwise RSIS_WGRAD_XCD=0 and =all on the same tiles stay inside the same bars.

All three knobs are read once per process, so every combination runs in a child process (this file, as a script; the children run
side by side); the defaults (the measured tables) run in the test process.  Every case is ONE rsis_conv2d_wgrad_batch call on top of
pre-filled dW.  The cases are the smallest that can go wrong (B <= 3, maps <= 32 x 32): rows and columns past the edge of a 128 tile,
every tile width, the three narrow-N classes of the 3x3, a launch whose jobs have block counts that are no multiples of 8 (the
permutation then crosses job boundaries; one job is a single block) and a group of more jobs than one launch holds."""
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

# a job: (B, [Cin segs], H, W, Cout, ks, lstm_hid); stride 1, "same" padding.  A case = the jobs of one grouped call.
_ONE = [
    # 1x1 at 16 x 16, Cout / Cs no multiples of 128: rows and columns past the edge of a 128 x 128 tile
    (2, [200], 16, 16, 72, 1, 0), (2, [72], 16, 16, 200, 1, 0), (2, [136], 16, 16, 264, 1, 0),
    # the bottleneck pair of layer 3
    (2, [256], 16, 16, 1024, 1, 0), (2, [1024], 16, 16, 256, 1, 0),
    # 1x1 on 32-wide tiles (8 x 32, 32 x 32) and on 8-wide ones (8 x 8)
    (2, [136], 8, 32, 200, 1, 0), (2, [160], 32, 32, 136, 1, 0), (3, [264], 8, 8, 136, 1, 0),
    # 3x3 with narrow N (N mod 128 in 1..64): Cout <= 32, <= 64, > 64 (the gate conv's second source), and a two-source gate conv with
    # 8 hidden channels; one narrow job on 8-wide tiles
    (2, [16], 16, 16, 32, 3, 0), (2, [48], 16, 16, 64, 3, 0), (2, [128, 64], 16, 16, 256, 3, 64), (2, [24, 8], 16, 16, 32, 3, 8),
    (2, [16], 8, 8, 96, 3, 0),
]
# eleven 3x3 jobs of one bucket (Cout > 64, N not narrow: the 128 x 128 tile under every rule, 16-wide spatial tiles of 4 rows).  With
# every block walking 2 spatial tiles (the group is far below the plan's block target) their block counts are
# 1, 12, 12, 6, 4, 9, 12, 2, 4, 3, 6 -- see _blocks_of_eleven
_ELEVEN = [(1, [8], 4, 16, 72, 3, 0), (3, [24], 16, 16, 72, 3, 0), (1, [40], 12, 16, 200, 3, 0), (1, [8], 20, 16, 136, 3, 0),
           (2, [56], 4, 16, 96, 3, 0), (1, [128], 4, 16, 72, 3, 0), (2, [24], 8, 16, 264, 3, 0), (1, [8], 12, 16, 72, 3, 0),
           (3, [8], 4, 16, 200, 3, 0), (1, [40], 4, 16, 72, 3, 0), (1, [24], 20, 16, 72, 3, 0)]
# fifty jobs of that bucket: more than one launch holds (RSIS_WG_MAXJ = 48)
_FIFTY = [(1 + i % 2, [8 if i % 3 else 24], 4 * (1 + i % 3), 16, 72 + 8 * (i % 4), 3, 0) for i in range(50)]
CASES = [[j] for j in _ONE] + [_ELEVEN, _FIFTY]


def _blocks_of_eleven():
    """block counts of _ELEVEN's jobs under the grouped split plan (tiles x ceil(spatial tiles / 2))"""
    out = []
    for B, segs, H, W, Cout, ks, hid in _ELEVEN:
        tiles = -(-Cout // 128) * -(-(segs[0] * 9) // 128)
        n_sp = B * (H // 4) * (W // 16)
        nsplit = -(-n_sp // 2)
        out.append(tiles * -(-n_sp // -(-n_sp // nsplit)))
    return out


def test_the_eleven_job_case_is_what_it_claims():
    b = _blocks_of_eleven()
    assert b == [1, 12, 12, 6, 4, 9, 12, 2, 4, 3, 6] and all(v % 8 for v in b) and sum(b) % 8 != 0
    for B, segs, H, W, Cout, ks, hid in _ELEVEN + _FIFTY:      # one bucket: the 128 x 128 tile under the single launch's rule
        n = segs[0] * 9 % 128
        assert Cout > 64 and (n == 0 or n > 64) and W == 16 and H % 4 == 0


def _rng_t(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, 1, shape).astype(np.float32))


def _inputs(k, i):
    B, segs, H, W, Cout, ks, hid = CASES[k][i]
    s = 100 * k + i
    xs = [_rng_t(300000 + 10 * s + n, (B, c, H, W)) for n, c in enumerate(segs)]
    return xs, _rng_t(500000 + s, (B, Cout, H, W)), _rng_t(700000 + s, (Cout, sum(segs), ks, ks))


def _reference(k):
    out = []
    for i, (B, segs, H, W, Cout, ks, hid) in enumerate(CASES[k]):
        xs, gy, prev = _inputs(k, i)
        wd = torch.zeros(Cout, sum(segs), ks, ks, dtype=torch.float64, requires_grad=True)
        F.conv2d(torch.cat(xs, 1).double(), wd, None, stride=1, padding=ks // 2).backward(gy.double())
        out.append(prev.double() + wd.grad)
    return out


def _run():
    """dW of every job (on top of its pre-filled contents), one rsis_conv2d_wgrad_batch call per case"""
    from rsis_amd import ops
    from rsis_amd._lib import WgradJob, check, lib, stream
    L = lib()
    res = []
    for k, case in enumerate(CASES):
        jobs, keep, out = [], [], []
        for i, (B, segs, H, W, Cout, ks, hid) in enumerate(case):
            xs, gy, prev = _inputs(k, i)
            if hid > 0:       # the kernel sees gate-interleaved dy rows 4 j + g and writes reference row g * hid + j
                gy = gy.reshape(B, 4, hid, H, W).transpose(1, 2).reshape(B, Cout, H, W).contiguous()
            dW, dy = prev.clone().cuda(), gy.cuda()
            c_off = 0
            for x in xs:
                xd = x.cuda()
                j = WgradJob()
                (j.dy, j.x, j.dW, j.B, j.Cs, j.H, j.W, j.Cout, j.Ho, j.Wo, j.ks, j.stride, j.pad, j.Ctot, j.c_off, j.lstm_hid, j.dtype) = (
                    dy.data_ptr(), xd.data_ptr(), dW.data_ptr(), B, x.shape[1], H, W, Cout, H, W, ks, 1, ks // 2, sum(segs), c_off, hid, ops.DTYPE_F32)
                jobs.append(j)
                keep.append(xd)
                c_off += x.shape[1]
            keep.append(dy)
            out.append(dW)
        arr = (WgradJob * len(jobs))(*jobs)
        check(L.rsis_conv2d_wgrad_batch(arr, len(jobs), stream()), "rsis_conv2d_wgrad_batch")
        torch.cuda.synchronize()
        res.append([t.cpu() for t in out])
    return res


def _run_all():
    from rsis_amd import ops
    res = {"run": _run()}
    prev = ops.set_deterministic(True)
    try:
        res["det_a"] = _run()
        res["det_b"] = _run()
    finally:
        ops.set_deterministic(prev)
    return res


# name -> (RSIS_WGRAD_TILES, RSIS_WGRAD_LIMBS, RSIS_WGRAD_XCD); None = unset
CHILDREN = {"base": ("0", "0", None), "wide_f32": ("wide", "0", None), "wide_limb": ("wide", "all", None),
            "wide_f32_x0": ("wide", "0", "0"), "wide_limb_x0": ("wide", "all", "0"),
            "wide_f32_xall": ("wide", "0", "all"), "wide_limb_xall": ("wide", "all", "all")}
KNOBS = ("RSIS_WGRAD_TILES", "RSIS_WGRAD_LIMBS", "RSIS_WGRAD_XCD")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wgrad_tiles")
    procs = {}
    for name, vals in CHILDREN.items():
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update({k: v for k, v in zip(KNOBS, vals) if v is not None})
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / (name + ".pt"))], env=env)
    try:
        res = {"ref": [_reference(k) for k in range(len(CASES))], "table": _run_all()}
        for name, p in procs.items():
            assert p.wait(timeout=600) == 0, "child %s failed" % name
            res[name] = torch.load(str(d / (name + ".pt")))
    finally:                      # whatever went wrong: no child goes on using the GPU
        for p in procs.values():
            if p.poll() is None:
                p.kill()
            p.wait()
    return res


def _err(got, ref):
    return [max(float((g.double() - r).abs().max()) for g, r in zip(gc, rc)) for gc, rc in zip(got, ref)]


def _bar(ref_case):
    return 2e-5 * max(1.0, max(float(r.abs().max()) for r in ref_case))


def _label(k):
    return repr(CASES[k][0]) if len(CASES[k]) == 1 else "%d jobs" % len(CASES[k])


WIDE = ["wide_f32", "wide_limb", "wide_f32_x0", "wide_limb_x0", "wide_f32_xall", "wide_limb_xall"]


@pytest.mark.parametrize("which", WIDE + ["table"])
def test_wide_tiles_against_float64_and_the_single_launch_rule(runs, which):
    ref = runs["ref"]
    e32, ew = _err(runs["base"]["run"], ref), _err(runs[which]["run"], ref)
    bad = []
    for k in range(len(CASES)):
        bar = _bar(ref[k])
        print("case %2d %-40s e32 %.3e  %s %.3e  ratio %.2f  bar %.3e" % (k, _label(k), e32[k], which, ew[k], ew[k] / max(e32[k], 1e-300), bar))
        if not (ew[k] <= 2.0 * e32[k] and ew[k] <= bar):
            bad.append((k, _label(k), e32[k], ew[k], bar))
    assert not bad, "beyond 2 x e32 or beyond 2e-5 * max(1, max |ref|): %r" % bad


@pytest.mark.parametrize("which", ["base"] + WIDE + ["table"])
def test_deterministic_mode_gives_equal_bits_twice(runs, which):
    for k in range(len(CASES)):
        for a, b in zip(runs[which]["det_a"][k], runs[which]["det_b"][k]):
            assert torch.equal(a, b), "case %d %s (%s): two deterministic calls differ" % (k, _label(k), which)
    ed = _err(runs[which]["det_a"], runs["ref"])
    for k in range(len(CASES)):
        assert ed[k] <= _bar(runs["ref"][k]), (k, _label(k), ed[k])


@pytest.mark.parametrize("other", ["", "_xall"], ids=["default", "all"])
@pytest.mark.parametrize("which", ["wide_f32", "wide_limb"])
def test_block_order_does_not_change_deterministic_bits(runs, which, other):
    for k in range(len(CASES)):
        for a, b in zip(runs[which + "_x0"]["det_a"][k], runs[which + other]["det_a"][k]):
            assert torch.equal(a, b), "case %d %s (%s): RSIS_WGRAD_XCD=0 differs from RSIS_WGRAD_XCD=%s" % (k, _label(k), which, other[2:] or "unset")


if __name__ == "__main__":
    torch.save(_run_all(), sys.argv[1])
