"""The dropout mask rule of include/rsis_hip.h (rsis_dropout_scales) as restated in numpy by rsis_amd/dropout.py, on the host: the
Philox4x32-10 known answers, and that the masks the GPU tests replay (dropout_cases.SEED) are not degenerate."""
import numpy as np
import pytest

import dropout_cases as C
from rsis_amd import dropout as D

PI = ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    (PI[0], PI[1], "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zero", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % int(v) for v in D.philox4x32_10(counter, key)) == want


def test_philox_broadcasts_over_counter_arrays():
    c0 = np.array([0, PI[0][0]], dtype=np.uint64)
    out = D.philox4x32_10((c0, PI[0][1], PI[0][2], PI[0][3]), PI[1])
    assert "%08x" % int(out[0][1]) == "d16cfe09" and int(out[0][0]) != int(out[0][1])


def test_scale_rule():
    st = C.state0()
    for p in (0.5, 0.3):
        m = D.scales_numpy(st, D.ARRAY_S2, 4096, p)
        keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        assert m.dtype == np.float32 and set(np.unique(m)) == {np.float32(0), keep}
        assert abs(float((m == 0).mean()) - p) < 0.03          # 4096 draws: 3 sigma is 0.023
    assert np.array_equal(D.scales_numpy(st, D.ARRAY_MC, 100, 0.0), np.ones(100, np.float32))
    # element e uses word e & 3 of block e >> 2; the arrays and the call counter are separate streams
    w = D.philox4x32_10((5, D.ARRAY_MS, 0, 0), (C.SEED, 0))
    m = D.scales_numpy(st, D.ARRAY_MS, 24, 0.5)
    for k in range(4):
        assert (m[20 + k] > 0) == (np.float32(int(w[k]) >> 8) * np.float32(2.0 ** -24) >= np.float32(0.5))
    assert not np.array_equal(D.scales_numpy(st, 0, 512, 0.5), D.scales_numpy(st, 1, 512, 0.5))
    assert not np.array_equal(D.scales_numpy(st, 0, 512, 0.5), D.scales_numpy(D.advance(st), 0, 512, 0.5))
    assert D.advance([1, 2, 0xFFFFFFFF, 0]) == [1, 2, 0, 1]


@pytest.mark.parametrize("rates", [(0.5, 0.5, 0.5), (0.3, 0.3, 0.3)], ids=["p0.5", "p0.3"])
@pytest.mark.parametrize("B", [2, 1])
def test_masks_of_the_gpu_tests_are_not_degenerate(rates, B):
    """at every level and in both head masks, every b has a kept and a dropped entry -- at the state the GPU tests start from and at the
    next one (their second draw)"""
    for st in (C.state0(), D.advance(C.state0())):
        for name, m in zip(("s2", "mc", "ms"), C.masks(st, rates, B=B)):
            assert C.nondegenerate(m, B=B), (name, st)


def test_ranks_draw_different_masks():
    for a, b in zip(C.masks(C.state0(0), (0.5, 0.5, 0.5)), C.masks(C.state0(1), (0.5, 0.5, 0.5))):
        assert not np.array_equal(a, b)
