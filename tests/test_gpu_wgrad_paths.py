"""A single weight gradient (rsis_conv2d_wgrad) runs as a group of one job on the grouped kernels of rsis_amd/csrc/conv_wgrad_tiled.hip
and conv_wgrad_bf16.hip; the build before that had single-launch kernels of its own.  In deterministic mode every dW element has one
contributor that walks the spatial tiles in order, so the bits are a function of the kernel, its tile and the block decomposition
alone, and this build must reproduce the parent build's bits on every launch path that was folded:

  * fp32 on aligned maps: one case per tile width of each kernel size; on ragged maps: RAG 1 and RAG 2; a ConvLSTM gate conv
    (two sources, gate-interleaved dy rows);
  * bf16 operands on fp32 storage (DTYPE_BF16): the _C3 + _C1 shapes of tests/test_gpu_wgrad_staged.py, which reach every
    (ks, BM, TW | BN, V4) instantiation of the register-staged kernels (test_every_instantiation_has_a_case there; the same wgb_key
    rule routes DTYPE_BF16 jobs);
  * blk operands (DTYPE_BF16_BLK): the DMA kernels at 8-, 16- and 32-wide tiles and every (BM, TW) -- the W3T_SHAPES of
    tests/test_gpu_blk.py with whole 8-channel blocks, without its 112^2 and 56^2 maps -- and the 1x1 at every (BM, BN).

Every family runs twice: job by job through rsis_conv2d_wgrad (the plain mode of wgb_find: one job, no lanes) and as ONE
rsis_conv2d_wgrad_batch call.  Everything here runs in deterministic mode, where rsis_conv2d_wgrad_batch (api.hip: the
`!rsis_deterministic()` condition in front of "grouped below") launches every job on its own: the batch call is one PLAIN-mode launch
per job, one split, like the single run beside it -- it checks the batch entry's routing, not the lane tables.  The lane mode of
wgb_find (default mode) is tests/test_gpu_wgrad_lanes.py.

The parent's dW is a dump that the parent build writes with this file as a script
(`RSIS_HIP_LIB=<parent library> python tests/test_gpu_wgrad_paths.py gpu_jobs/wgrad_paths_parent_dw.pt`), a measurement, not a
golden; the comparison skips when there is none.  The bf16 kernels also have to give equal bits in two calls of this build, and
their deterministic results, single and batch, lie within the ROUNDING bar of tests/wgrad_lane_cases.py around float64: one block walks
every tile of its job here, so |err_ij| <= n 2^-23 (|prev_ij| + A_ij), the worst case of any fp32 summation of exactly representable
terms (A: the float64 weight gradient of |dy|, |x| rounded to bf16; n = B H W)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_wgrad_staged import _C1, _C3  # noqa: E402

pytestmark = pytest.mark.gpu

# family -> [(B, [Cin segs], H, W, Cout, ks, lstm_hid)]; every conv is stride 1, "same" padding
CASES = {
    "fp32_aligned": [(2, [16], 16, 16, 32, 3, 0), (2, [32], 16, 16, 128, 3, 0), (2, [256], 16, 16, 64, 1, 0), (2, [64], 8, 32, 96, 1, 0)],
    "fp32_ragged": [(2, [8], 9, 11, 16, 3, 0), (2, [16], 28, 28, 32, 3, 0)],
    "fp32_convlstm": [(2, [24, 8], 16, 16, 32, 3, 8)],
    "bf16": _C3 + _C1,
    "blk": [(3, [40], 14, 14, 24, 3, 0), (5, [16], 7, 7, 8, 3, 0), (2, [64], 28, 28, 48, 3, 0), (2, [64], 16, 16, 64, 1, 0),
            # W3T_SHAPES of tests/test_gpu_blk.py with Cin % 8 == 0 and Cout % 8 == 0 (the first two are the two cases above)
            (2, [520], 28, 28, 72, 3, 0), (2, [520], 14, 14, 72, 3, 0), (3, [520], 7, 7, 72, 3, 0), (8, [128], 7, 7, 128, 3, 0),
            (3, [48], 33, 20, 16, 3, 0), (2, [72], 5, 11, 136, 3, 0),
            # one 1x1 per (BM, BN)
            (2, [64], 8, 8, 64, 1, 0), (2, [64], 8, 8, 136, 1, 0), (2, [136], 8, 8, 64, 1, 0), (2, [136], 8, 8, 136, 1, 0)],
}
FAMILIES = list(CASES)
PARENT_DUMP = os.path.join(ROOT, "gpu_jobs", "wgrad_paths_parent_dw.pt")


def _rng_t(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, 1.0, shape).astype(np.float32))


def _blk(t):
    """NCHW fp32 -> channel-blocked bf16 [B][C / 8][H][W][8]"""
    B, C, H, W = t.shape
    return t.reshape(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)


def _run(grouped=False):
    """deterministic-mode dW of every case, on top of pre-filled contents, through rsis_conv2d_wgrad or (grouped) one
    rsis_conv2d_wgrad_batch call per family: {family: [dW, ...]}"""
    from rsis_amd import ops
    from rsis_amd._lib import WgradJob, check, lib, ptr, stream
    L = lib()
    out = {}
    prev_mode = ops.set_deterministic(True)
    try:
        for f, family in enumerate(FAMILIES):
            dtype = {"bf16": ops.DTYPE_BF16, "blk": ops.DTYPE_BF16_BLK}.get(family, ops.DTYPE_F32)
            out[family] = []
            jobs, keep = [], []
            for k, (B, segs, H, W, Cout, ks, hid) in enumerate(CASES[family]):
                seed = 100 * f + 10 * k
                Ctot = sum(segs)
                gy = _rng_t(31000 + seed, (B, Cout, H, W))
                if hid > 0:       # the kernel sees gate-interleaved dy rows 4 j + g and writes reference row g * hid + j
                    gy = gy.reshape(B, 4, hid, H, W).transpose(1, 2).reshape(B, Cout, H, W).contiguous()
                dy = (_blk(gy) if family == "blk" else gy).cuda()
                dW = _rng_t(32000 + seed, (Cout, Ctot, ks, ks)).cuda()
                c_off = 0
                for i, c in enumerate(segs):
                    x = _rng_t(33000 + seed + i, (B, c, H, W))
                    xd = (_blk(x) if family == "blk" else x).cuda()
                    if grouped:
                        j = WgradJob()
                        (j.dy, j.x, j.dW, j.B, j.Cs, j.H, j.W, j.Cout, j.Ho, j.Wo, j.ks, j.stride, j.pad, j.Ctot, j.c_off, j.lstm_hid, j.dtype) = (
                            dy.data_ptr(), xd.data_ptr(), dW.data_ptr(), B, c, H, W, Cout, H, W, ks, 1, ks // 2, Ctot, c_off, hid, dtype)
                        jobs.append(j)
                        keep.append(xd)
                    else:
                        check(L.rsis_conv2d_wgrad(ptr(dy), ptr(xd), ptr(dW), B, c, H, W, Cout, H, W, ks, 1, ks // 2, Ctot, c_off, hid, dtype,
                                                  stream()), "rsis_conv2d_wgrad")
                    c_off += c
                keep.append(dy)
                out[family].append(dW)
            if grouped:
                check(L.rsis_conv2d_wgrad_batch((WgradJob * len(jobs))(*jobs), len(jobs), stream()), "rsis_conv2d_wgrad_batch")
            torch.cuda.synchronize()
            out[family] = [t.cpu() for t in out[family]]
    finally:
        ops.set_deterministic(prev_mode)
    return out


def _run_all():
    out = _run()
    out.update({"grouped_" + f: v for f, v in _run(True).items()})
    return out


@pytest.fixture(scope="module")
def runs():
    return _run_all(), _run_all()


@pytest.mark.parametrize("family", FAMILIES)
def test_single_launch_reproduces_the_parent_build(runs, family):
    if not os.path.exists(PARENT_DUMP):
        pytest.skip("no dump of the parent build's dW at gpu_jobs/wgrad_paths_parent_dw.pt")
    parent = torch.load(PARENT_DUMP)
    assert len(parent[family]) == len(CASES[family])
    for c, a, b in zip(CASES[family], runs[0][family], parent[family]):
        assert torch.isfinite(a).all() and torch.equal(a, b), "%s case %r: the deterministic dW differs from the parent build's" % (family, c)


@pytest.mark.parametrize("family", FAMILIES)
def test_grouped_launch_reproduces_the_parent_build(runs, family):
    if not os.path.exists(PARENT_DUMP):
        pytest.skip("no dump of the parent build's dW at gpu_jobs/wgrad_paths_parent_dw.pt")
    parent = torch.load(PARENT_DUMP)
    assert len(parent["grouped_" + family]) == len(CASES[family])
    for c, a, b in zip(CASES[family], runs[0]["grouped_" + family], parent["grouped_" + family]):
        assert torch.isfinite(a).all() and torch.equal(a, b), "%s case %r: the grouped deterministic dW differs from the parent build's" % (family, c)


@pytest.mark.parametrize("family", ["bf16", "blk"])
def test_bf16_single_launch_is_deterministic(runs, family):
    for c, a, b in zip(CASES[family], runs[0][family], runs[1][family]):
        assert torch.isfinite(a).all() and torch.equal(a, b), "%s case %r: two deterministic calls differ" % (family, c)


@pytest.mark.parametrize("family", ["bf16", "blk"])
def test_bf16_grouped_launch_is_deterministic(runs, family):
    for c, a, b in zip(CASES[family], runs[0]["grouped_" + family], runs[1]["grouped_" + family]):
        assert torch.isfinite(a).all() and torch.equal(a, b), "%s case %r: two deterministic grouped calls differ" % (family, c)


def _wgrad64(dy, x, Cout, ks):
    w = torch.zeros(Cout, x.shape[1], ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, stride=1, padding=ks // 2).backward(dy)
    return w.grad


@pytest.fixture(scope="module")
def float64_terms():
    """{family: [(prev + g, n 2^-23 (|prev| + A)), ...]} of the bf16 and blk families, float64, on the inputs of _run rounded to bf16 (round
    to nearest even; the blk operands are those values already)"""
    out = {}
    for f, family in enumerate(FAMILIES):
        if family not in ("bf16", "blk"):
            continue
        out[family] = []
        for k, (B, segs, H, W, Cout, ks, hid) in enumerate(CASES[family]):
            seed = 100 * f + 10 * k
            gy = _rng_t(31000 + seed, (B, Cout, H, W)).bfloat16().double()            # (reference row order: g * hid + j)
            prev = _rng_t(32000 + seed, (Cout, sum(segs), ks, ks)).double()
            x = torch.cat([_rng_t(33000 + seed + i, (B, c, H, W)) for i, c in enumerate(segs)], 1).bfloat16().double()
            g, A = _wgrad64(gy, x, Cout, ks), _wgrad64(gy.abs(), x.abs(), Cout, ks)
            out[family].append((prev + g, B * H * W * 2.0 ** -23 * (prev.abs() + A)))
    return out


@pytest.mark.parametrize("mode", ["single", "batch"])
@pytest.mark.parametrize("family", ["bf16", "blk"])
def test_bf16_deterministic_results_against_float64(runs, float64_terms, family, mode):
    from helpers import assert_close
    got = runs[0][family if mode == "single" else "grouped_" + family]
    assert len(got) == len(CASES[family])
    for c, a, (ref, bar) in zip(CASES[family], got, float64_terms[family]):
        err = a.double() - ref
        assert_close("%s %s case %r: |err| / ROUNDING (max |err| %.3e)" % (family, mode, c, float(err.abs().max())), err / bar,
                     torch.zeros_like(err), 1.0)


if __name__ == "__main__":
    torch.save(_run_all(), sys.argv[1])
