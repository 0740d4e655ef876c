"""Host side of test_gpu_blk_paths.py: the rounding helpers against torch's own bfloat16 conversion, the preconditions of the exact regimes
(sum |terms| below 2^24, representable / tie shares), the launch rules the case tables restate, the 1 % cap on the undecided share of
every normal case -- and that the checkers CAN fail: the numpy fp32 model of an op with one defect at a time is rejected at every case
the defect applies to, the honest model passes."""
import numpy as np
import pytest
import torch

import blk_paths_cases as K

F32 = np.float32


def _torch_bf16(a32):
    return torch.from_numpy(np.asarray(a32, F32)).to(torch.bfloat16).double().numpy()


# ---------------------------------------------------------------- rounding helpers
def test_bf16_rne64_matches_torch_on_fp32_values():
    """ties, both fp32 neighbours of a tie, binade boundaries, +-0, +-inf, NaN, denormals, the largest finite values; and a seeded sweep"""
    v = K.from_nchw_specials()
    rng = np.random.default_rng(0)
    sweep = (rng.standard_normal(200000) * np.exp2(rng.integers(-140, 128, 200000).astype(np.float64))).astype(F32).astype(np.float64)
    for a in (v, sweep[np.isfinite(sweep)]):
        got, want = K.bf16_rne64(a), _torch_bf16(a)
        nan = np.isnan(a)
        assert np.isnan(got[nan]).all() and np.isnan(want[nan]).all()
        assert np.array_equal(got[~nan], want[~nan])
        assert np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan])), "the sign of zero"
    assert K.bf16_rne64([float(np.finfo(F32).max)])[0] == np.inf and K.bf16_rne64([K._BF16_MAX])[0] == K._BF16_MAX


def test_bf16_rne64_rounds_once_where_float32_on_the_way_would_round_twice():
    a = np.array([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    assert K.bf16_rne64(a).tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0, 1.0 + 2.0 ** -6]
    assert _torch_bf16(a.astype(F32)).tolist()[0] == 1.0, "through float32 the first value becomes the tie and goes to even"


def test_mid_dist_and_neighbours():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 - 2.0 ** -9, 2.0 - 2.0 ** -8, 300.0, 301.0, -301.0, 0.0, 2.0 ** -134])
    assert K.mid_dist(a).tolist() == [2.0 ** -9, 0.0, 2.0 ** -9, 0.0, 0.0, 1.0, 0.0, 0.0, 2.0 ** -134, 0.0]
    lo, hi = K.bf16_neighbours(np.array([301.0, -301.0, 1.0, 2.0 - 2.0 ** -8]))
    assert lo.tolist() == [300.0, -300.0, 1.0, 2.0 - 2.0 ** -7] and hi.tolist() == [302.0, -302.0, 1.0 + 2.0 ** -7, 2.0]
    assert K.is_tie(np.array([301.0, 300.0, 1.0 + 2.0 ** -8])).tolist() == [True, False, True]
    assert K.trunc_bf16(np.array([301.9, -301.9])).tolist() == [300.0, -300.0]
    assert K.half_away_bf16(np.array([301.0, 303.0, -301.0, 300.9])).tolist() == [302.0, 304.0, -302.0, 300.0]
    assert K.bf16_rne64(np.array([301.0, 303.0])).tolist() == [300.0, 304.0]


def test_nearest_check_rules():
    ref = np.array([300.6, 301.0 - 1e-6, 301.0 - 1e-6, 301.0 - 1e-6, 0.0, 0.0, 5.0])
    got = np.array([300.0, 300.0, 302.0, 304.0, 0.0, 2.0 ** -133, 5.0])
    assert K.nearest_check(got, ref, 1e-5).tolist() == [True, True, True, False, True, False, True]
    assert K.nearest_check(got, ref, 1e-7).tolist() == [True, True, False, False, True, False, True]
    assert K.nearest_check(np.array([-0.0]), np.array([0.0]), 0.0).all(), "an exact zero behind a ReLU, either sign"
    assert K.undecided(ref, 1e-5).tolist() == [False, True, True, True, False, False, False]
    with pytest.raises(AssertionError):
        K.assert_nearest("x", got, ref, 1e-7)
    K.assert_nearest("x", got, ref, 1e-7, where=np.array([1, 1, 0, 0, 1, 0, 1], bool))


def test_guarded_blk_sees_a_write_on_either_side():
    g = K.GuardedBlk((2, 1, 3, 3, 8), device="cpu")
    assert g.t.dtype == torch.bfloat16 and g.t.data_ptr() % 16 == 0 and K.GUARD_BLK >= 64 and g.untouched()
    assert float(g.t.float().abs().min()) > 0, "the prefill is non-zero"
    g.check()
    g.t.fill_(1.0)
    g.check()
    assert not g.untouched()
    for i in (K.GUARD_BLK - 1, K.GUARD_BLK + g.n):
        h = K.GuardedBlk((2, 1, 3, 3, 8), device="cpu")
        h.buf[i] = 0
        with pytest.raises(AssertionError):
            h.check()


# ---------------------------------------------------------------- convs, exact regime
_CONV = {}


def _conv_data(c):
    k = K.conv_id(c)
    if k not in _CONV:
        _CONV[k] = K.conv_exact_data(c)
    return _CONV[k]


def test_conv_case_table_covers_the_launch_rules():
    nq3 = sorted({-(-c["Cin"] // 16) for c in K.CONV_CASES if c["ks"] == 3})
    nq1 = sorted({-(-c["Cin"] // 32) for c in K.CONV_CASES if c["ks"] == 1})
    assert nq3[:4] == [1, 2, 3, 4] and nq3[-1] >= 16 and nq1[:5] == [1, 2, 3, 4, 5] and nq1[-1] >= 32
    assert {24, 40} <= {c["Cin"] for c in K.CONV_CASES if c["ks"] == 3}, "ragged last stage at nq 2 and nq 3"
    for ks in (1, 3):
        cs = [c for c in K.CONV_CASES if c["ks"] == ks]
        assert {8, 24, 40, 64, 136} <= {c["Cout"] for c in K.CONV_CASES}
        assert any(c["role"] == "round" for c in cs), "one rounding case per kernel family"
        assert any(c["H"] * c["W"] == 1 for c in cs), "a 1 x 1 map"
    maps = {(c["H"], c["W"]) for c in K.CONV_CASES}
    assert {(5, 5), (9, 11), (10, 13), (17, 9), (1, 1)} <= maps
    w3 = [c["W"] for c in K.CONV_CASES if c["ks"] == 3]
    assert min(w3) <= 8 and any(8 < w <= 16 for w in w3) and max(w3) > 16, "the three dispatch branches of variant 0, 3x3"
    p1 = [c["H"] * c["W"] for c in K.CONV_CASES if c["ks"] == 1]
    assert min(p1) <= 64 < max(p1) and 99 in p1 and 153 in p1
    tiles = [c["B"] * -(-c["H"] // 8) * -(-c["W"] // 8) for c in K.CONV_CASES if c["ks"] == 3]
    assert any(t % 8 for t in tiles), "a number of pixel tiles that is no multiple of 8"
    assert all(c["why"] for c in K.CONV_CASES) and len({K.conv_id(c) for c in K.CONV_CASES}) == len(K.CONV_CASES)


@pytest.mark.parametrize("c", K.CONV_CASES, ids=K.conv_id)
def test_conv_exact_cases_are_exact_and_serve_their_role(c):
    d = _conv_data(c)
    for k in ("x", "w", "dy", "add"):
        assert np.abs(d[k]).max() <= 3 and np.array_equal(d[k], np.round(d[k]))
    assert d["abs_y"].max() < 2 ** 24 and d["abs_dx"].max() < 2 ** 24, "the fp32 accumulation is exact in any order"
    assert np.abs(d["y"]).max() > 0
    if c["role"] == "index":
        assert K.is_bf16(d["y"]).all() and K.is_bf16(d["dx"]).all() and d["abs_y"].max() <= 2 ** 11
    if c["role"] == "round":
        assert (~K.is_bf16(d["y"])).mean() >= K.MIN_NOT_BF16, (~K.is_bf16(d["y"])).mean()
    if c["role"] in ("round", "tie"):
        assert K.is_tie(d["y"]).mean() >= K.MIN_TIES, K.is_tie(d["y"]).mean()


def _conv_taps(x, w, drop=None, halo_zero=False):
    """direct float64 conv by taps (the defect models: one tap of one input channel dropped / the map's last halo-adjacent column read as 0)"""
    B, Cin, H, W = x.shape
    Cout, _ci, ks, _ = w.shape
    p = ks // 2
    xp = np.zeros((B, Cin, H + 2 * p, W + 2 * p))
    xp[:, :, p:p + H, p:p + W] = x
    y = np.zeros((B, Cout, H, W))
    for r in range(ks):
        for s in range(ks):
            win = xp[:, :, r:r + H, s:s + W]
            wt = w[:, :, r, s].copy()
            if drop == (r, s):
                wt[:, Cin - 1] = 0.0
            t = np.einsum("bchw,oc->bohw", win, wt)
            if halo_zero and s == 0 and ks == 3:      # the left neighbour of the first column of a second 8-wide tile: read as zero
                col = min(8, W - 1)
                t[:, :, :, col] = 0.0
            y += t
    return y


@pytest.mark.parametrize("c", K.CONV_CASES, ids=K.conv_id)
def test_conv_defects_are_rejected(c):
    """equality with bf16_rne64(reference) rejects: a dropped tap of one channel, a halo column read as zero"""
    d = _conv_data(c)
    honest = _conv_taps(d["x"], d["w"])
    assert np.array_equal(honest, d["y"])
    want = K.bf16_rne64(d["y"])
    centre = (c["ks"] // 2, c["ks"] // 2)
    assert not np.array_equal(K.bf16_rne64(_conv_taps(d["x"], d["w"], drop=centre)), want)
    if c["ks"] == 3 and c["W"] > 1:
        assert not np.array_equal(K.bf16_rne64(_conv_taps(d["x"], d["w"], halo_zero=True)), want)


@pytest.mark.parametrize("c", [c for c in K.CONV_CASES if c["role"] in ("round", "tie")], ids=K.conv_id)
def test_conv_rounding_defects_are_rejected(c):
    """truncation and half-away-from-zero each change a rounding case"""
    d = _conv_data(c)
    want = K.bf16_rne64(d["y"])
    assert not np.array_equal(K.trunc_bf16(d["y"]), want)
    assert not np.array_equal(K.half_away_bf16(d["y"]), want)
    # (two roundings cannot show on integers with two bits below the bf16 grid; they are pinned by the two modes of bn_eval below and
    #  rejected on the BatchNorm's normal data)


@pytest.mark.parametrize("c", K.BATCH_CASES, ids=K.batch_id)
def test_batch_exact_cases_are_exact_and_serve_their_role(c):
    d = K.batch_exact_data(c)
    assert d["abs_yb"].max() < 2 ** 24 and d["abs_dx"].max() < 2 ** 24 and np.abs(d["bias"]).max() <= 3
    assert all(v % 8 == 0 for v in c["segs"]) and (c["split"] is None or (sum(c["split"]) == c["Cout"] and all(v % 8 == 0 for v in c["split"])))
    if c["role"] == "index":
        assert K.is_bf16(d["y"]).all() and K.is_bf16(d["yb"]).all() and K.is_bf16(d["dx0"]).all()
        assert K.is_bf16(d["y"] + d["bias"][None, :, None, None]).all() and K.is_bf16(d["y"] + d["add_out"]).all()
    else:
        assert (~K.is_bf16(d["yb"])).mean() >= K.MIN_NOT_BF16 and K.is_tie(d["yb"]).mean() >= K.MIN_TIES
        assert not np.array_equal(K.trunc_bf16(d["yb"]), K.bf16_rne64(d["yb"])) and not np.array_equal(K.half_away_bf16(d["yb"]), K.bf16_rne64(d["yb"]))


def test_batch_case_table():
    assert [c["segs"] for c in K.BATCH_CASES[:3]] == [[8], [24, 8, 40], [16, 8]] and set(K.BATCH_TILES) == {0, 1, 4, 5}
    assert any(c["split"] and c["split"][0] % 32 for c in K.BATCH_CASES), "a destination boundary that is no multiple of 32 rows"
    assert any(c["W"] > 16 for c in K.BATCH_CASES) and any(c["role"] == "round" for c in K.BATCH_CASES)


@pytest.mark.parametrize("state", [False, True], ids=["zero", "recurrent"])
@pytest.mark.parametrize("c", K.LSTM_CASES, ids=K.lstm_id)
def test_lstm_cases_are_exact_decidable_and_reject_a_truncating_store(c, state):
    """every gate pre-activation exact in fp32 (multiples of 1 / 32, sum |terms| below 2^19) and |pre| <= 8 for 90 %; at most 1 % of h and of
    act undecided under the E_F deltas (third rule on at most 0.5 %); the fp32 model of the epilogue passes every check of the GPU test,
    a truncating store of h or act is rejected"""
    d = K.lstm_data(c, state)
    assert np.array_equal(d["pre"] * 32, np.round(d["pre"] * 32)) and d["abs_pre"].max() * 32 < 2 ** 24
    assert (np.abs(d["pre"]) <= 8).mean() >= 0.9 and np.abs(d["c"]).max() <= 2.0
    if state:
        assert np.abs(d["c_prev"]).max() <= 1 and K.is_bf16(d["h_prev"]).all()
    dh, da = K.lstm_delta_h(d["c"]), K.E_F
    for ref, delta in ((d["h"], dh), (d["act"], da)):
        assert K.undecided(ref, delta).mean() <= K.UNDECIDED_CAP, K.undecided(ref, delta).mean()
        assert wide_share(ref, np.broadcast_to(delta, ref.shape)) <= WIDE_CAP
    c32, h32, a32 = K.lstm_model32(d)
    assert (np.abs(c32 - d["c"]) <= K.lstm_delta_c(d["c"])).all()
    K.assert_nearest("model h", K.bf16_rne64(h32), d["h"], dh)
    K.assert_nearest("model act", K.bf16_rne64(a32), d["act"], da)
    for store in (K.trunc_bf16, _twice):
        assert not K.nearest_check(store(h32), d["h"], dh).all() and not K.nearest_check(store(a32), d["act"], da).all(), store.__name__


def test_lstm_case_table_and_probe_grid():
    assert sorted(c["hid"] for c in K.LSTM_CASES) == [8, 16, 24] and set(K.LSTM_TILES) == {4, 5} and any(c["c_up"] == 0 for c in K.LSTM_CASES)
    v = K.fast_probe_args()
    assert v.min() == -24 and v.max() == 24 and 0.0 in v and len(v) >= 600
    for c in K.LSTM_CASES:
        for state in (False, True):
            pre = K.lstm_data(c, state)["pre"]
            inside = np.abs(pre) <= 24
            assert inside.all() and np.isin(pre, v).all(), "the probe covers EVERY pre-activation of the cases"
    assert np.isin(K.lstm_pre_values(), v).all() and np.abs(K.lstm_pre_values()).max() <= 8


def test_side_key_cases_and_the_tie_rule():
    """the case table against RSIS_SIDE_CHECK_TILES; exact pre-activations; the key order prefers the larger value, then the SMALLER pixel
    -- and a pooling that keeps the last of two equal maxima is rejected by `pixel == 0` on the tie data"""
    assert [K.side_tiles(c) for c in K.SIDE_CASES] == [2, K.SIDE_CHECK_TILES, 176] and K.SIDE_CASES[0]["hid"] == 24
    for c in K.SIDE_CASES:
        for tie in (True, False):
            d = K.side_data(c, tie)
            assert np.array_equal(d["pre"] * 16, np.round(d["pre"] * 16)) and np.abs(d["pre"]).max() < 2 ** 8, "exact in fp32"
            assert (np.abs(d["pre"]) <= 8).mean() >= 0.9
            h = d["h"].reshape(c["B"], c["hid"], -1)
            # the deltas of the GPU test (E_F chain): at most 1 % undecided, the third rule on at most 0.5 %; the fp32 model passes
            dh = K.lstm_delta_h(d["c"])
            for ref, delta in ((d["h"], dh), (d["act"], K.E_F)):
                assert K.undecided(ref, delta).mean() <= K.UNDECIDED_CAP, (K.side_id(c), tie, K.undecided(ref, delta).mean())
                assert wide_share(ref, np.broadcast_to(delta, ref.shape)) <= WIDE_CAP
            c32, h32, a32 = K.lstm_model32(dict(d, c_prev=None))
            assert (np.abs(c32 - d["c"]) <= K.lstm_delta_c(d["c"])).all()
            K.assert_nearest("model h", K.bf16_rne64(h32), d["h"], dh)
            K.assert_nearest("model act", K.bf16_rne64(a32), d["act"], K.E_F)
            if tie:
                assert (h == h[:, :, :1]).all() and float(np.abs(h).max()) > 0.05
            elif c["csrc"]:
                assert (h.max(2) > np.median(h, 2)).all(), "a non-trivial maximum"
    v = np.array([0.5, 0.5, -0.25, 0.75, 0.75], F32)
    keys = K.key_encode(v, np.arange(5))
    val, idx = K.key_decode(keys.astype(np.int64))
    assert np.array_equal(val, v.astype(np.float64)) and idx.tolist() == [0, 1, 2, 3, 4]
    assert int(np.argmax(keys)) == 3 and keys[0] > keys[1] > keys[2]
    # the defect -- a pooling that keeps the LAST of equal maxima -- through the GPU test's checks on the tie data of every case
    for c in K.SIDE_CASES:
        h32 = K.side_data(c, True)["h"].reshape(c["B"], c["hid"], -1).astype(F32)
        hs = K.bf16_rne64(h32.astype(np.float64))
        for last in (False, True):
            pix = h32.shape[2] - 1 - np.argmax(h32[:, :, ::-1], 2) if last else np.argmax(h32, 2)
            keys = K.key_encode(np.take_along_axis(h32, pix[:, :, None], 2)[:, :, 0], pix)
            val, idx = K.key_decode(keys.astype(np.int64))
            at = np.take_along_axis(hs, idx[:, :, None], 2)[:, :, 0]
            assert np.array_equal(at, K.bf16_rne64(val)) and np.array_equal(at, hs.max(2)), "the value checks cannot see the defect"
            assert bool((idx == 0).all()) == (not last), "`idx == 0` must pass the first maximum and reject the last"


@pytest.mark.parametrize("c", K.BN_EVAL_CASES, ids=K.conv_id)
def test_bn_eval_modes_have_exact_and_different_expectations(c):
    d, p = _conv_data(c), K.bn_eval_params(c)
    for k in ("gamma", "var", "sc"):
        m, _e = np.frexp(np.abs(p[k]))
        assert (m == 0.5).all(), "%s: powers of two" % k
    m, _e = np.frexp(np.abs(p["sh"][p["sh"] != 0]))
    assert (m == 0.5).all() and set(p["var"].tolist()) <= set(K.RSQRT_POW2)
    assert np.array_equal(p["sc"], p["gamma"] / np.sqrt(p["var"])) and np.array_equal(p["sh"], p["beta"] - p["mean"] * p["sc"])
    for relu in (False, True):
        for res in (None, p["res"]):
            e0, e1 = K.bn_eval_expect(d["y"], p, res, relu, 0), K.bn_eval_expect(d["y"], p, res, relu, 1)
            # the affine map is exact in fp32: the unrounded value has at most 24 significant bits
            o = d["y"] * p["sc"][None, :, None, None] + p["sh"][None, :, None, None] + (0.0 if res is None else res)
            assert np.array_equal(o.astype(F32).astype(np.float64), o)
            if not relu:
                assert (e0 != e1).mean() >= K.BN_EVAL_MIN_DIFF, (e0 != e1).mean()
            assert not np.array_equal(K.bn_eval_expect(d["y"], p, res, relu, 1, store=K.trunc_bf16), e1)


# ---------------------------------------------------------------- BatchNorm
def test_bn_case_table_restates_the_launch_rules():
    assert [c["B"] * c["H"] * c["W"] for c in K.BN_CASES] == [2, 135, 2048, 2049, 4096, 4097, 6272, 25088, 75264]
    for c in K.BN_CASES:
        plan = K.bn_plan(c["B"], c["C"], c["H"], c["W"])
        for k, v in c["expect"].items():
            assert plan[k] == v, (K.bn_id(c), k, plan[k], v)
        assert c["C"] % 8 == 0 and plan["S"] <= 64 and c["B"] * c["C"] * c["H"] * c["W"] * 2 < 10e6, "every bf16 buffer under 10 MB"
    assert sorted({K.bn_plan(c["B"], c["C"], c["H"], c["W"])["S"] for c in K.BN_CASES}) == [1, 5, 7, 25, 59]
    assert 1.0 <= K.M_BN <= 4.0 and K.K_RSTD_ULP == 1.0 + np.ceil(K.R_RSQRT) + 1.0


def test_wave_sums_follow_the_kernels_order():
    """wave_sums against explicit loops over threads, cells and fold steps, both kernel families; and the sequential chain for comparison"""
    rng = np.random.default_rng(5)
    for c in (K.BN_CASES[3], K.BN_CASES[5]):
        plan = K.bn_plan(c["B"], c["C"], c["H"], c["W"])
        N = plan["N"]
        a = (rng.standard_normal((1, N)) * 2 + 16).astype(F32)
        T, p, blocks = (512, plan["NPT"], 1) if plan["kernel"] == "block" else (256, plan["per"] // 256, plan["S"])
        total = 0.0
        for blk in range(blocks):
            v = np.zeros(T, F32)
            for t in range(T):
                for j in range(p):
                    n = blk * T * p + j * T + t
                    if n < min(N, (blk + 1) * T * p):
                        v[t] = F32(v[t] + a[0, n])
            for w in range(T // 64):
                lane = v[w * 64:(w + 1) * 64].copy()
                for o in (32, 16, 8, 4, 2, 1):
                    lane = np.array([F32(lane[i] + lane[i ^ o]) for i in range(64)], F32)
                total += float(lane[0])
        assert K.wave_sums(a, plan)[0] == total
        assert abs(K.chain_sums(a, plan["chain"])[0] - a.astype(np.float64).sum()) < 1e-2 * N


_BN = {}


def _bn_data(c, regime):
    k = (K.bn_id(c), regime)
    if k not in _BN:
        _BN[k] = K.bn_inputs(c, regime)
    return _BN[k]


@pytest.mark.parametrize("regime", sorted(K.BN_EXACT_SETS))
@pytest.mark.parametrize("c", K.BN_CASES, ids=K.bn_id)
def test_bn_exact_sums_stay_below_2_to_24(c, regime):
    """no fp32 accumulation of the launch crosses a block: a block kernel's block holds the whole channel, a two-pass block one split of
    `per` cells; blocks and splits meet in double.  So sum |x|, sum x^2 and sum |dy| (|xhat| <= ... is not exact: only dbeta is demanded)
    over any `block_cells` consecutive cells bound every fp32 chain -- below 2^24 all of them are exact integers."""
    d = _bn_data(c, regime)
    plan = K.bn_plan(c["B"], c["C"], c["H"], c["W"])
    x = d["x"].transpose(1, 0, 2, 3).reshape(c["C"], -1)
    assert np.array_equal(x, np.round(x)) and np.array_equal(d["dy"], np.round(d["dy"]))
    lo, hi = K.BN_EXACT_SETS[regime]
    assert plan["block_cells"] * max(lo * lo, hi * hi) < 2 ** 24, "the stated chain bound: block_cells x max x^2"
    pad = (-x.shape[1]) % plan["block_cells"]
    q = np.concatenate([x * x, np.zeros((c["C"], pad))], 1).reshape(c["C"], -1, plan["block_cells"]).sum(2)
    assert q.max() < 2 ** 24 and np.abs(d["dy"]).sum((0, 2, 3)).max() < 2 ** 24
    assert (x * x).sum(1).max() < 2 ** 53 and np.abs(d["db0"]).max() <= 5
    if regime == "far" and plan["N"] > 2:
        st = K.bn_stats64(d["x"])
        assert (st["mean"] / np.sqrt(st["var"])).min() > 7.0, "a mean of about 8 standard deviations"


def _bars(d, c, relu, res):
    """(f, b, model, e) of a normal case: float64 forward / backward (mask of the model's stored y), the honest model and M_BN x its errors"""
    f = K.bn_fwd64(d, relu, res)
    m = K.bn_model32(d, c, relu, res)
    b = K.bn_bwd64(d, f["st"], m["mask"])
    e = {k: K.M_BN * v for k, v in K.bn_sum_errors(m, f, b).items()}
    return f, b, m, e


def _twice(a):
    """defect model: two roundings -- first to a grid four times finer than bf16 (half to even), then to bf16"""
    lo, hi = K.bf16_neighbours(a)
    q = (hi - lo) / 4
    return K.bf16_rne64(lo + np.rint((np.asarray(a, np.float64) - lo) / q) * q)


def wide_share(ref, delta):
    """share of the elements to which nearest_check's third rule (delta above half a bf16 step) applies"""
    lo, hi = K.bf16_neighbours(ref)
    return float(((np.asarray(ref) != 0) & (delta > np.abs(hi - lo) / 2)).mean())


WIDE_CAP = 0.005                      # nearest_check's third rule may apply to at most half of the undecided cap (its elements are undecided too)


@pytest.mark.parametrize("regime", sorted(K.BN_NORMAL_SETS))
@pytest.mark.parametrize("relu,res", [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize("c", K.BN_CASES, ids=K.bn_id)
def test_bn_normal_cases_are_decidable_and_reject_the_defects(c, regime, relu, res):
    """EVERY normal case, from the reference alone, with the deltas of the GPU test (M_BN x err_host): at most 1 % of y and of dx within
    delta of a midpoint, nearest_check's third rule on at most 0.5 %; the honest fp32 model passes.  Then one defect at a time on the
    model's unrounded fp32 results, through the comparisons the GPU test makes: a truncating store and two roundings are rejected on y and
    dx at every case above two cells (16 elements hold too few double roundings), and -- relu -- the mask
    taken from the unrounded value with the sign flipped at the smallest positive result by `dres == dy * (stored y > 0)`."""
    d = _bn_data(c, regime)
    f, b, m, e = _bars(d, c, relu, res)
    N = c["B"] * c["H"] * c["W"]
    dy_ = K.bn_delta_y(d, f, res, e["mean"], e["rstd"])
    assert K.undecided(f["y"], dy_).mean() <= K.UNDECIDED_CAP, K.undecided(f["y"], dy_).mean()
    assert wide_share(f["y"], dy_) <= WIDE_CAP, wide_share(f["y"], dy_)
    K.assert_nearest("model y", m["y"], f["y"], dy_)
    # (half away from zero differs from nearest-even only where the fp32 result IS a midpoint; the reference is then within delta of it and
    #  nearest_check accepts both neighbours by design: that defect is rejected in the exact regime -- test_bn_eval_tie_data_rejects_...)
    for store in (K.trunc_bf16,) + ((_twice,) if N > 2 else ()):
        assert not K.nearest_check(store(m["y32"]), f["y"], dy_).all(), "y: %s passes" % store.__name__
    if relu:
        pos = np.where(m["pre32"] > 0, m["pre32"], np.inf)
        bad_mask = m["pre32"] > 0
        bad_mask.reshape(-1)[int(np.argmin(pos))] = False
        stored = m["y"] > 0
        assert np.array_equal(m["dres"], d["dy"] * stored), "the honest dres passes the GPU test's comparison"
        assert not np.array_equal(K.bf16_rne64(d["dy"] * bad_mask), d["dy"] * stored), "the defective mask passes it"
    if N <= 2:
        return                                                      # two cells: dx is pure cancellation, compared absolutely on the device
    ddx = K.bn_delta_dx(d, f["st"], b, e["mean"], e["rstd"], e["dbeta"], e["dgamma"])
    assert K.undecided(b["dx"], ddx).mean() <= K.UNDECIDED_CAP, K.undecided(b["dx"], ddx).mean()
    assert wide_share(b["dx"], ddx) <= WIDE_CAP, wide_share(b["dx"], ddx)
    K.assert_nearest("model dx", m["dx"], b["dx"], ddx)
    for store in (K.trunc_bf16, _twice):
        assert not K.nearest_check(store(m["dx32"]), b["dx"], ddx).all(), "dx: %s passes" % store.__name__
    clear = K.clear_of_zero(f["pre"], relu)
    assert clear.mean() > 0.9 and np.array_equal(m["mask"][clear], (f["pre"] > 0)[clear] if relu else m["mask"][clear])


@pytest.mark.parametrize("regime", sorted(K.BN_EXACT_SETS))
@pytest.mark.parametrize("c", K.BN_CASES[1:], ids=K.bn_id)
def test_bn_statistics_defects_are_rejected_by_the_exact_bars(c, regime):
    """a cell dropped at a split boundary, and N - 1 in place of N, move save_mean by far more than its 1-ulp bar at every shape"""
    d = _bn_data(c, regime)
    st = K.bn_stats64(d["x"])
    plan = K.bn_plan(c["B"], c["C"], c["H"], c["W"])
    ulp = np.spacing(np.abs(st["mean"]).astype(F32)).astype(np.float64)
    honest = K.bn_model32(dict(d, dy=None), c, False, False)
    assert (np.abs(honest["mean"] - st["mean"]) <= ulp).all()
    assert (np.abs(honest["rstd"] - st["rstd"]) <= K.K_RSTD_ULP * np.spacing(st["rstd"].astype(F32))).all()
    cell = min(plan["per"], plan["N"]) - 1                          # the last cell of the first split
    for kw in (dict(drop_cell=cell), dict(n_minus_1=True)):
        bad = K.bn_model32(dict(d, dy=None), c, False, False, **kw)
        ch = np.abs(d["x"].transpose(1, 0, 2, 3).reshape(c["C"], -1)[:, cell] - st["mean"]) > 0.25 if "drop_cell" in kw else st["mean"] != 0
        assert ch.any() and (np.abs(bad["mean"] - st["mean"])[ch] > 8 * ulp[ch]).all(), kw


def test_bn_eval_tie_data_rejects_half_away_and_truncation():
    """the exact-regime BatchNorm store check (eval mode, sc = 1, sh = 1/2 on integers 128..255): every unrounded output is a tie"""
    d = K.bn_tie_data()
    assert K.is_tie(d["y"]).all() and np.array_equal(d["y"].astype(F32).astype(np.float64), d["y"])
    want = K.bf16_rne64(d["y"])
    for store in (K.trunc_bf16, K.half_away_bf16):
        assert not np.array_equal(store(d["y"]), want)
    assert (K.half_away_bf16(d["y"]) != want).mean() > 0.4


# ---------------------------------------------------------------- layout helpers
def test_from_nchw_specials_cover_what_they_claim():
    v = K.from_nchw_specials()
    fin = v[np.isfinite(v)]
    assert K.is_tie(fin).sum() >= 40 and np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
    assert (np.abs(fin[fin != 0]) < 2.0 ** -126).sum() >= 10 and np.signbit(v[v == 0]).any() and (~np.signbit(v[v == 0])).any()
    assert float(np.finfo(F32).max) in v.tolist()
