"""Host side of test_gpu_train_paths.py: the preconditions of its exact regime, the dispatch rules its case table restates, the data-gradient
extension of the summation-order models, and the cost of its largest float64 reference."""
import time

import numpy as np
import pytest
import torch

import train_paths_cases as T
from helpers import host_sums, host_sums_conv, host_sums_dgrad

FWD_EXACT = T.DIRECT_EXACT + T.SPLIT_FWD + T.S2_EXACT + T.IGEMM_FWD_EXACT + T.C1_EXACT
DGRAD_EXACT = T.DIRECT_DGRAD_EXACT + T.SPLIT_DGRAD + T.S2_EXACT + T.IGEMM_DGRAD_EXACT + T.C1_EXACT


def test_exact_regime_stays_below_2_to_24():
    """sum |terms| < 2^24 for every output of every exact case: fp32 sums of such integers are exact in any order"""
    for cases, dgrad in ((FWD_EXACT, False), (DGRAD_EXACT, True)):
        for c in cases:
            assert T.exact_bound(c, dgrad) < T.EXACT_LIMIT, T.case_id(c)
            assert c["why"]
    # the bound is a bound: the measured sum of |terms| of one forward and one gradient case
    c = T.DIRECT_EXACT[0]
    d = T.fwd_data(c, "exact", 1)
    tot = torch.nn.functional.conv2d(torch.from_numpy(np.abs(d["xs"][0])).double(), torch.from_numpy(np.abs(d["w"])).double(), padding=1)
    assert float(tot.max()) + 6 <= T.exact_bound(c)
    assert all(float(np.abs(a).max()) <= 3 for a in (d["xs"][0], d["w"], d["b"], d["add"]))
    assert d["ref"].dtype == torch.float64 and float((d["ref"] - d["ref"].round()).abs().max()) == 0.0
    g = T.dgrad_data(T.IGEMM_DGRAD_EXACT[3], "exact", 2)
    assert float(np.abs(g["add"]).min()) >= 1, "the prefill of the in-place scatter has no zero"


def test_split_k_cases_give_the_slices_their_comments_claim():
    """launch_direct_cfg()'s ksplit and the api.hip gate, restated in train_paths_cases.py, against the `slices` / `seg` fields of the table.
    A retuned rule in conv3x3_direct.hip or api.hip fails here: update the restated rule AND the cases (each must still cross its edge)."""
    for c, dgrad in [(c, False) for c in T.SPLIT_FWD] + [(c, True) for c in T.SPLIT_DGRAD]:
        for tile in (0, 1):                                  # the dispatcher picks variant 1 for each of them
            variant, ks, sl, seg = T.split_plan(c, tile, dgrad)
            assert variant == 1 and sl == c["slices"] and ks == len(c["slices"]) and seg == c["seg"], (T.case_id(c), variant, ks, sl, seg)
        assert 0 in c["tiles"] and 1 in c["tiles"]
    assert T.slice_chunks(33, 4) == [8, 8, 8, 9] and T.chunks([257]) == 33 and 257 % T.CK == 1
    big = [c for c in T.SPLIT_FWD if c["seg"]][0]
    assert min(big["slices"]) >= T.FLUSH_MIN_CHUNKS
    for v in (4, 5, 6):                                      # the 32-row variants: 256 blocks, unsplit, segmented over all 192 chunks
        assert T.split_plan(big, v)[1:] == (1, [192], True)
    assert T.split_plan(big, 9)[1:] == (4, [48] * 4, False)  # a 512-thread variant: split, no segmented instantiation
    for c in T.SPLIT_FWD:                                    # deterministic mode: unsplit, the dispatcher's choice is variant 6
        assert T.split_plan(c, 0, deterministic=True) == (6, 1, [T.chunks(c["segs"])], T.chunks(c["segs"]) >= T.FLUSH_MIN_CHUNKS)
    # a data gradient with an addend is never split; below 32 chunks nothing is
    assert T.split_plan(dict(T.SPLIT_DGRAD[0], addend=True), 1, True)[1] == 1
    assert T.split_plan(T._c("", 2, [248], 8, 8, 40), 1)[1] == 1
    # the igemm dispatcher's own tile: codes 11 and 16 are reached by no case's own choice -- they are forced (IGEMM_TILES)
    assert {11, 12, 15, 16} <= set(T.IGEMM_TILES) and set(range(1, 7)) <= set(T.IGEMM_TILES)


def _brute_dgrad(dy, w, stride, pad, Hx, Wx):
    """dx by the definition, fp32, terms added in the order (co ascending, r' then s' ascending with r = ks-1-r', s = ks-1-s')"""
    B, Cout, Hy, Wy = dy.shape
    Cin, ks = w.shape[1], w.shape[2]
    dx = np.zeros((B, Cin, Hx, Wx), np.float32)
    for b in range(B):
        for ci in range(Cin):
            for y in range(Hx):
                for x in range(Wx):
                    acc = np.float32(0)
                    for co in range(Cout):
                        for rp in range(ks):
                            for sp in range(ks):
                                r, s = ks - 1 - rp, ks - 1 - sp
                                ty, tx = y + pad - r, x + pad - s
                                if ty % stride or tx % stride or not (0 <= ty // stride < Hy and 0 <= tx // stride < Wy):
                                    continue
                                acc = np.float32(acc + np.float32(dy[b, co, ty // stride, tx // stride] * w[co, ci, r, s]))
                    dx[b, ci, y, x] = acc
    return dx


@pytest.mark.parametrize("shape", [(1, 11, 3, 3, 1, 1, 5, 4), (2, 10, 2, 3, 2, 1, 5, 6), (1, 9, 2, 1, 2, 0, 5, 4)],
                         ids=["3x3s1", "3x3s2_odd_x_even", "1x1s2"])
def test_host_sums_dgrad_against_a_brute_force_loop(shape):
    B, Cout, Cin, ks, stride, pad, Hx, Wx = shape
    Hy, Wy = (Hx + 2 * pad - ks) // stride + 1, (Wx + 2 * pad - ks) // stride + 1
    dy, w = T.normal(1, (B, Cout, Hy, Wy)), T.normal(2, (Cout, Cin, ks, ks), 0.3)
    chain, seg = host_sums_dgrad(dy, w, stride, pad, Hx, Wx)
    brute = _brute_dgrad(dy, w, stride, pad, Hx, Wx)
    assert np.array_equal(chain, brute), "the chain is the brute-force loop's order: equal bits"
    ref = torch.nn.functional.conv_transpose2d(torch.from_numpy(dy).double(), torch.from_numpy(w).double(), stride=stride, padding=pad,
                                               output_padding=(Hx - ((Hy - 1) * stride - 2 * pad + ks), Wx - ((Wy - 1) * stride - 2 * pad + ks))).numpy()
    assert np.abs(chain - ref).max() < 1e-5 and np.abs(seg - ref).max() < 1e-5
    assert np.array_equal(seg, chain)                        # <= 4 chunks of dy rows: no segment boundary


def test_host_sums_dgrad_segments_count_chunks_of_dy_rows():
    dy, w = T.normal(3, (1, 40, 4, 4)), T.normal(4, (40, 2, 3, 3), 0.1)
    chain, seg = host_sums_dgrad(dy, w, 1, 1, 4, 4)
    assert not np.array_equal(chain, seg)                    # 5 chunks: one boundary
    lo, _ = host_sums_dgrad(dy[:, :32], w[:32], 1, 1, 4, 4)
    hi, _ = host_sums_dgrad(dy[:, 32:], w[32:], 1, 1, 4, 4)
    assert np.array_equal(seg, lo + hi)


def test_host_sums_conv_generalises_host_sums():
    xs = [T.normal(5, (2, 20, 5, 6)), T.normal(6, (2, 21, 5, 6))]
    w, b = T.normal(7, (3, 41, 3, 3), 0.1), T.normal(8, (3,))
    for got, want in zip(host_sums_conv(xs, w, b, 1, 1), host_sums(xs, w, b)):
        assert np.array_equal(got, want)
    # stride 2 / pad 1: the stride-1 outputs at the even pixels, the same chain
    c2, _ = host_sums_conv(xs, w, b, 2, 1)
    assert np.array_equal(c2, host_sums(xs, w, b)[0][:, :, ::2, ::2])
    x7, w7 = T.normal(9, (1, 3, 9, 7)), T.normal(10, (4, 3, 7, 7), 0.1)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x7).double(), torch.from_numpy(w7).double(), stride=2, padding=3).numpy()
    assert np.abs(host_sums_conv([x7], w7, None, 2, 3)[0] - ref).max() < 1e-5


def test_largest_reference_is_cheap():
    """the float64 reference of the largest case (and its host models over TIGHT_IMAGES images) in a few seconds"""
    big = max(FWD_EXACT, key=lambda c: c["B"] * sum(c["segs"]) * c["cout"] * c["ks"] ** 2 * T.out_size(c)[0] * T.out_size(c)[1])
    t0 = time.perf_counter()
    d = T.fwd_data(big, "normal", 1)
    t_ref = time.perf_counter() - t0
    n = T.TIGHT_IMAGES
    host_sums_conv([x[:n] for x in d["xs"]], d["w"], d["b"], 1, 1)
    t_all = time.perf_counter() - t0
    print("largest case %s: float64 reference %.2f s, with the host models %.2f s" % (T.case_id(big), t_ref, t_all))
    assert t_ref < 5.0 and t_all < 10.0
