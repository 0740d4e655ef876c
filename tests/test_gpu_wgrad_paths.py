"""A single weight gradient (rsis_conv2d_wgrad) runs as a group of one job on the grouped kernels of rsis_amd/csrc/conv_wgrad_tiled.hip
and conv_wgrad_bf16.hip; the build before that had single-launch kernels of its own.  In deterministic mode every dW element has one
contributor that walks the spatial tiles in order, so the bits are a function of the kernel, its tile and the block decomposition
alone, and this build must reproduce the parent build's bits on every launch path that was folded:

  * fp32 on aligned maps: one case per tile width of each kernel size; on ragged maps: RAG 1 and RAG 2; a ConvLSTM gate conv
    (two sources, gate-interleaved dy rows);
  * bf16 operands on fp32 storage (DTYPE_BF16): 3x3 and 1x1, W % 4 (1x1: H * W % 4) both ways;
  * blk operands (DTYPE_BF16_BLK): the DMA kernels at 8-, 16- and 32-wide tiles, and the 1x1.

The parent's dW is a dump that the parent build writes with this file as a script
(`RSIS_HIP_LIB=<parent library> python tests/test_gpu_wgrad_paths.py gpu_jobs/wgrad_paths_parent_dw.pt`), a measurement, not a
golden; the comparison skips when there is none.  The bf16 kernels also have to give equal bits in two calls of this build."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# family -> [(B, [Cin segs], H, W, Cout, ks, lstm_hid)]; every conv is stride 1, "same" padding
CASES = {
    "fp32_aligned": [(2, [16], 16, 16, 32, 3, 0), (2, [32], 16, 16, 128, 3, 0), (2, [256], 16, 16, 64, 1, 0), (2, [64], 8, 32, 96, 1, 0)],
    "fp32_ragged": [(2, [8], 9, 11, 16, 3, 0), (2, [16], 28, 28, 32, 3, 0)],
    "fp32_convlstm": [(2, [24, 8], 16, 16, 32, 3, 8)],
    "bf16": [(2, [16], 16, 16, 32, 3, 0), (2, [64], 14, 14, 64, 3, 0), (2, [64], 16, 16, 128, 1, 0), (3, [40], 7, 7, 24, 1, 0)],
    "blk": [(3, [40], 14, 14, 24, 3, 0), (5, [16], 7, 7, 8, 3, 0), (2, [64], 28, 28, 48, 3, 0), (2, [64], 16, 16, 64, 1, 0)],
}
FAMILIES = list(CASES)
PARENT_DUMP = os.path.join(ROOT, "gpu_jobs", "wgrad_paths_parent_dw.pt")


def _rng_t(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, 1.0, shape).astype(np.float32))


def _blk(t):
    """NCHW fp32 -> channel-blocked bf16 [B][C / 8][H][W][8]"""
    B, C, H, W = t.shape
    return t.reshape(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)


def _run():
    """deterministic-mode dW of every case, on top of pre-filled contents, through rsis_conv2d_wgrad: {family: [dW, ...]}"""
    from rsis_amd import ops
    from rsis_amd._lib import check, lib, ptr, stream
    L = lib()
    out = {}
    prev_mode = ops.set_deterministic(True)
    try:
        for f, family in enumerate(FAMILIES):
            dtype = {"bf16": ops.DTYPE_BF16, "blk": ops.DTYPE_BF16_BLK}.get(family, ops.DTYPE_F32)
            out[family] = []
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
                    check(L.rsis_conv2d_wgrad(ptr(dy), ptr(xd), ptr(dW), B, c, H, W, Cout, H, W, ks, 1, ks // 2, Ctot, c_off, hid, dtype, stream()),
                          "rsis_conv2d_wgrad")
                    c_off += c
                torch.cuda.synchronize()
                out[family].append(dW.cpu())
    finally:
        ops.set_deterministic(prev_mode)
    return out


@pytest.fixture(scope="module")
def runs():
    return _run(), _run()


@pytest.mark.parametrize("family", FAMILIES)
def test_single_launch_reproduces_the_parent_build(runs, family):
    if not os.path.exists(PARENT_DUMP):
        pytest.skip("no dump of the parent build's dW at gpu_jobs/wgrad_paths_parent_dw.pt")
    parent = torch.load(PARENT_DUMP)
    assert len(parent[family]) == len(CASES[family])
    for c, a, b in zip(CASES[family], runs[0][family], parent[family]):
        assert torch.isfinite(a).all() and torch.equal(a, b), "%s case %r: the deterministic dW differs from the parent build's" % (family, c)


@pytest.mark.parametrize("family", ["bf16", "blk"])
def test_bf16_single_launch_is_deterministic(runs, family):
    for c, a, b in zip(CASES[family], runs[0][family], runs[1][family]):
        assert torch.isfinite(a).all() and torch.equal(a, b), "%s case %r: two deterministic calls differ" % (family, c)


if __name__ == "__main__":
    torch.save(_run(), sys.argv[1])
