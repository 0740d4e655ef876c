"""The two host models of the fp32 summation order that the bars of test_gpu_infer_paths.py rest on (`chain` and `segmented`, numpy only),
checked where no GPU is needed: the chunk count runs on across the sources, and on a single source of 47 / 48 / 49 chunks the segmented
sum leaves 0.21 / 0.25 / 0.21 of the chain's error against float64 -- the figures the "at most half the chain's error" assertion of the
GPU tests is set against."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import f32_normal as _rng, host_sums as _host_sums, max_err as _err, to_tensor as _t


def test_host_models_count_chunks_like_the_kernel():
    """sources [20, 12]: 3 + 2 chunks, the segment boundary after the first 8 channels of the second source (chunk 4), none inside [32]"""
    x = [_rng(1, (1, 20, 3, 3)), _rng(2, (1, 12, 3, 3))]
    w = _rng(3, (2, 32, 3, 3))
    chain, seg = _host_sums(x, w, None)
    head, _ = _host_sums([x[0], x[1][:, :8]], w[:, :28], None)         # chunks 0..3 as one chain
    tail, _ = _host_sums([x[1][:, 8:]], w[:, 28:], None)               # chunk 4
    assert np.array_equal(seg, head + tail) and not np.array_equal(seg, chain)
    chain, seg = _host_sums([np.concatenate(x, 1)], w, None)
    assert np.array_equal(seg, chain)


@pytest.mark.parametrize("C,chain_err,ratio", [(32, 2.1e-6, 1.00), (72, 3.6e-6, 0.57), (376, 7.4e-6, 0.21), (384, 6.6e-6, 0.25), (392, 6.2e-6, 0.21)])
def test_segmented_to_chain_error_ratio(C, chain_err, ratio):
    """B = 2, a 9 x 13 map, 40 output channels, one source of C channels (seeds 1 and 2); numpy's fp32 arithmetic is deterministic, so
    the figures are reproduced to the digits they are quoted with"""
    x, w = _rng(1, (2, C, 9, 13)), _rng(2, (40, C, 3, 3), 1.0 / np.sqrt(9 * C))
    ref = F.conv2d(_t(x).double(), _t(w).double(), None, padding=1)
    chain, seg = _host_sums([x], w, None)
    e_chain, e_seg = _err(chain, ref), _err(seg, ref)
    assert abs(e_chain - chain_err) <= 0.06e-6 and abs(e_seg / e_chain - ratio) <= 0.006, (e_chain, e_seg / e_chain)
