"""heads_wide_cases.py and the dispatch rule of the class / stop heads (ops.heads_family, decoder_seq.supported) without a device."""
import numpy as np
import pytest

import heads_wide_cases as W
import loss_path_cases as L
from helpers import mk_args


@pytest.mark.parametrize("s", W.EXACT_SHAPES, ids=L.heads_id)
def test_exact_shapes_are_exact_and_new_ground(s):
    """every sum of |terms| of the exact case stays below 2^24 (so fp32 is exact in any order), and the small kernels refuse the shape"""
    assert L.heads_exact_bound(L.heads_exact_data(s)) < 2 ** 24
    assert not L.heads_fits(s[0], sum(s[1]), s[2])


def test_family_rule_restates_the_small_kernels_limits():
    """ops.heads_family: "small" exactly where rsis_heads_bwd's rule (loss_path_cases.heads_fits) accepts, the forward wherever ncls <= 64,
    "wide" up to 1024 classes and 2048 features, nothing beyond; the bench's heads stay on the small family"""
    from rsis_amd import ops
    for K in (1, 24, 248, 2048):
        for ncls in (1, 9, 21, 64, 65, 81, 1024):
            for rows in (1, 2, 64, 65, 320, 364, 365, 640, 2600):
                want = "small" if L.heads_fits(rows, K, ncls) else "wide"
                assert ops.heads_family(rows, K, ncls, backward=True) == want, (rows, K, ncls)
                assert ops.heads_family(rows, K, ncls) == ("small" if ncls <= L.HEADS_MAXC else "wide"), (rows, K, ncls)
    assert ops.heads_family(320, 248, 21) == "small" and ops.heads_family(320, 248, 21, backward=True) == "small"
    assert ops.heads_family(32, 248, 21, backward=True) == "small"
    for bad in ((0, 248, 21), (4, 2049, 21), (4, 0, 21), (4, 248, 1025), (4, 248, 0)):
        assert ops.heads_family(*bad) is None and ops.heads_family(*bad, backward=True) is None


def _probes(B, hs=128, blk=False):
    from rsis_amd import decoder_seq
    sizes = [(8, 8), (16, 16), (32, 32), (64, 64), (128, 128)]
    chans = [hs, hs, hs // 2, hs // 4, hs // 8]
    return [decoder_seq.ShapeProbe(B, c, h, w, blk and i < 4) for i, (c, (h, w)) in enumerate(zip(chans, sizes))]


@pytest.mark.parametrize("ncls,B,want", [(21, 32, True), (64, 32, True), (65, 32, True), (81, 32, True), (21, 65, True), (21, 1, True),
                                         (1024, 2, True), (1025, 32, False), (81, 4096, True)])
def test_sequence_decoder_accepts_wide_heads(ncls, B, want):
    from rsis_amd import decoder_seq
    from rsis_amd.modules import RSIS
    dec = RSIS(mk_args(num_classes=ncls))
    assert decoder_seq.supported(dec, _probes(B), 10) == want


def test_sequence_decoder_bf16_accepts_81_classes():
    from rsis_amd import decoder_seq
    from rsis_amd.modules import RSIS
    dec = RSIS(mk_args(num_classes=81, dtype="bf16"))
    assert decoder_seq.supported_for_input(dec, [128, 128, 64, 32, 16], 32, 256, 256, 20)
    assert not decoder_seq.supported_for_input(RSIS(mk_args(num_classes=1025, dtype="bf16")), [128, 128, 64, 32, 16], 32, 256, 256, 20)


def test_single_step_heads_keep_the_batch_of_one_quirk():
    """ops.heads_supported: a batch of one stays with the reference's statement in single-step RSIS.forward; only the sequence asks min_rows=1"""
    from rsis_amd import decoder_seq, ops
    from rsis_amd.modules import RSIS
    dec = RSIS(mk_args(num_classes=81))
    one, two = [decoder_seq.ShapeProbe(1, 128, 8, 8, False)], [decoder_seq.ShapeProbe(2, 128, 8, 8, False)]
    assert not ops.heads_supported(one * 5, dec.fc_class, dec.fc_stop)
    assert ops.heads_supported(one * 5, dec.fc_class, dec.fc_stop, min_rows=1)
    assert ops.heads_supported(two * 5, dec.fc_class, dec.fc_stop)


def test_bounds_are_positive_and_small():
    """the a priori bounds of a normal case: finite, positive, and far below the values they bound (a bound of the size of the value
    would check nothing)"""
    s = (70, [24, 8], 81)
    d = L.heads_normal_data(s, "normal")
    pb, sb = W.fwd_bounds(d)
    assert np.isfinite(pb).all() and (pb > 0).all() and (pb <= 1e-3 * d["probs"] + 2 * W.TINY).all()
    assert (sb > 0).all() and sb.max() < 1e-4
    b = W.bwd_bounds(d)
    ref = d["ref"]
    for k in ("dside", "dWc", "dbc", "dWs", "dbs"):
        assert np.isfinite(b[k]).all() and (b[k] > 0).all() and b[k].shape == np.asarray(ref[k]).shape, k
        assert b[k].max() <= 1e-3 * max(np.abs(ref[k]).max(), 1e-3), k
    # the host model of the small kernels (one sequential fp32 chain per sum) must itself lie within them
    assert (np.abs(d["host"]["probs"].astype(np.float64) - d["probs"]) <= pb).all()
    assert (np.abs(d["host"]["stop"].astype(np.float64) - d["stop"]) <= sb).all()
    assert (np.abs(d["host"]["dside"].astype(np.float64) - ref["dside"]) <= b["dside"]).all()
    assert (np.abs(d["host"]["dW"][:81].astype(np.float64) - ref["dWc"]) <= b["dWc"]).all()
