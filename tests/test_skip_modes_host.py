"""Host tests of `-skip_mode sum | mul | none` on the sequence decoder: the column offsets of the gate packs and the channel rule of
decoder_seq.supported against their restatement in skip_mode_cases.py, and the float64 references of the GPU kernel tests against
plain torch (F.interpolate(align_corners=True) * m and its autograd)."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_cases as R
import skip_mode_cases as S


@pytest.mark.parametrize("key", sorted(S.PACK_OFFSETS, key=str), ids=lambda k: "%s-%d-%d" % k)
def test_pack_offsets_per_mode(key):
    from rsis_amd import decoder_fused
    mode, c_up, c_skip = key
    assert decoder_fused.pack_offsets(c_up, c_skip, mode) == S.PACK_OFFSETS[key]


def test_pack_offsets_refuse_what_no_mode_defines():
    from rsis_amd import decoder_fused
    with pytest.raises(ValueError):
        decoder_fused.pack_offsets(64, 32, "sum")          # a sum of tensors with different channel counts
    with pytest.raises(ValueError):
        decoder_fused.pack_offsets(64, 64, "bogus")


class _Cell(object):
    """what decoder_fused._packs reads of a ConvLSTMCell"""

    def __init__(self, hid):
        self.hidden_size, self.kernel_size, self.padding, self._packs = hid, 3, 1, {}


@pytest.mark.parametrize("mode", S.MODES)
def test_packs_carry_the_offsets_and_hoist_only_where_the_mode_is_linear(mode):
    """the pack constructor runs without a device: segments and offsets of the pair per level of the reference's pyramid"""
    from rsis_amd import decoder_fused
    for level, (cin, c_up, c_skip) in enumerate(S.level_channels(128, mode)):
        cell = _Cell(128 >> level)
        hid = cell.hidden_size
        hoist, dyn = decoder_fused._packs(cell, c_up, c_skip, mode)
        skip_off, h_off = decoder_fused.pack_offsets(c_up, c_skip, mode)
        if level == 0 or mode in ("concat", "sum"):
            assert hoist is not None and hoist.segs == [c_skip] and hoist.offs == [skip_off]
        else:
            assert hoist is None
        assert dyn.segs == ([c_up] if c_up else []) + [hid] and dyn.offs == ([0] if c_up else []) + [h_off]
        assert h_off == cin, "the h_prev columns follow the cell's input channels"
        assert decoder_fused._packs(cell, c_up, c_skip, mode)[1] is dyn, "the pair is cached on the cell"
        # the copies the node derives from the dynamic pack follow its segments
        assert decoder_fused.dyn_fwd_pack(cell, c_up, c_skip, None, False, mode) is dyn
    # concat keeps the key it had before the modes existed (the per-step path looks the pair up without a mode)
    cell = _Cell(64)
    assert decoder_fused._packs(cell, 128, 128) is decoder_fused._packs(cell, 128, 128, "concat")
    assert list(cell._packs) == [("fused", 128, 128, 0)]


@pytest.mark.parametrize("case", S.CHANNEL_RULE, ids=lambda c: "%s-%d-%d-%d" % c[:4])
def test_channel_rule(case):
    from rsis_amd import decoder_seq
    mode, cin, c_up, c_skip, want = case
    assert decoder_seq.channels_ok(mode, cin, c_up, c_skip) is want


def _probe_decoder(mode, hidden=32, dropout=0.0):
    """an RSIS on the host (its constructor allocates no device memory) -- supported() reads only attributes and shapes of it"""
    from helpers import mk_args
    from rsis_amd.modules import RSIS
    return RSIS(mk_args(hidden_size=hidden, skip_mode=mode, dropout=dropout))


@pytest.mark.parametrize("mode", S.MODES)
def test_supported_through_shape_probes(mode):
    from rsis_amd import decoder_seq
    if not decoder_seq.ENABLED[0]:
        pytest.skip("RSIS_DECODER_SEQ=0")
    dec = _probe_decoder(mode)
    ch = S.skip_channels(32)
    probes = [decoder_seq.ShapeProbe(2, c, h, w, False) for c, (h, w) in zip(ch, S.PYRAMID)]
    assert decoder_seq.supported(dec, probes, 3) is True
    # one skip feature with half its channels: concat, sum and mul refuse the pyramid, none never reads the feature's channels
    probes[2] = decoder_seq.ShapeProbe(2, ch[2] // 2, S.PYRAMID[2][0], S.PYRAMID[2][1], False)
    assert decoder_seq.supported(dec, probes, 3) is (mode == "none")


def test_mul_with_dropout2d_stays_on_the_per_step_path():
    from rsis_amd import decoder_seq
    if not decoder_seq.ENABLED[0]:
        pytest.skip("RSIS_DECODER_SEQ=0")
    probes = [decoder_seq.ShapeProbe(2, c, h, w, False) for c, (h, w) in zip(S.skip_channels(32), S.PYRAMID)]
    assert decoder_seq.supported(_probe_decoder("mul", dropout=0.5), probes, 3) is False
    assert decoder_seq.supported(_probe_decoder("sum", dropout=0.5), probes, 3) is True
    assert decoder_seq.supported(_probe_decoder("none", dropout=0.5), probes, 3) is True


# ---------------------------------------------------------------- the float64 references of the kernel tests
@pytest.mark.parametrize("c", S.MUL_FWD, ids=R.case_id)
def test_mul_references_against_torch(c):
    m, (dy,) = S.mul_operands(c, 1)
    r = R.up_fwd_refs(c)
    x = torch.from_numpy(r["x"]).double()[None].requires_grad_()
    mt = torch.from_numpy(m).double()[None].requires_grad_()
    y = F.interpolate(x, size=(c["Ho"], c["Wo"]), mode="bilinear", align_corners=True) * mt
    y.backward(torch.from_numpy(dy).double()[None])
    want, bar = S.mul_fwd_ref(c, m)
    assert np.array_equal(want, y.detach()[0].numpy())
    assert bar.shape == want.shape and bool((bar >= 0).all()) and bool((bar[np.abs(want) > 0] > 0).all())
    dym, dm = S.mul_prep_ref(c, m, dy)
    assert np.allclose(dm, mt.grad[0].numpy(), rtol=1e-14, atol=0)
    # dy * m is what the unscaled transpose is then applied to: d x = resize^T(dy * m)
    x0 = torch.from_numpy(r["x"]).double()[None].requires_grad_()
    F.interpolate(x0, size=(c["Ho"], c["Wo"]), mode="bilinear", align_corners=True).backward(torch.from_numpy(dym)[None])
    assert np.allclose(x0.grad.numpy(), x.grad.numpy(), rtol=1e-12, atol=1e-300)


def test_the_case_lists_cover_every_launch_path_once():
    paths = [c["path"] for c in S.MUL_FWD]
    assert set(paths) == set(c["path"] for c in R.UP_FWD)
    assert len(paths) <= len(set(paths)) + 1, "one case per path; the second identity case may share its path with another"
    assert sum(1 for c in S.MUL_FWD if c.get("identity")) == 2
    for c in S.MUL_FWD:
        assert R.upsample_fwd_path(c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]) == c["path"]
    assert {c["path"] == "scalar" for c in S.MUL_PREP} == {True, False}, "the preparation's float4 and scalar paths"


def test_fma32_is_one_rounding():
    rs = np.random.default_rng(5)
    a, b = rs.normal(0, 1, 4000).astype(np.float32), rs.normal(0, 1, 4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * np.float32(1 + 2.0 ** -12)    # heavy cancellation
    c[::2] = rs.normal(0, 1, 2000).astype(np.float32)
    # a tie of the float64 sum that the exact residual breaks: a * b = 1 + 2^-24 + 2^-48 exactly, c = 0 -> above the midpoint of fp32
    a[0], b[0], c[0] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-(2.0 ** -11) + 2.0 ** -24)
    got = S.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))           # float(Fraction) rounds once to float64; bracket with the fp32 neighbours
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)
