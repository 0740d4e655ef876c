"""Host side of test_gpu_loss_path.py: the preconditions of its exact regimes, the launch rules its case tables restate, the host models
against brute-force loops, that every normal case HAS a yardstick (err_host finite and non-zero), and the cost of the references."""
import time

import numpy as np
import pytest

import loss_path_cases as L

F32 = np.float32


# ---------------------------------------------------------------- exact-regime preconditions
def test_three_logits_have_exact_fp32_sigmoids():
    """-100, 0, +30 under 1 / (1 + exp(-x)) in fp32: exactly 0, 1/2, 1 -- and p (1 - p) exactly 0, 1/4, 0"""
    p = L.sigmoid32(np.array(L.EXACT_LOGITS, F32))
    assert p.dtype == F32 and p.tolist() == [0.0, 0.5, 1.0]
    assert (p * (F32(1) - p)).tolist() == [0.0, 0.25, 0.0]
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(F32(100.0), dtype=F32))
    assert F32(1) + np.exp(F32(-30.0), dtype=F32) == F32(1)


def test_exact_sums_are_halves_below_2_to_23():
    """every exact S is a multiple of 1/2 and N < 2^23 halves: an fp32 sum of such terms is exact in any order and under any atomics"""
    for c in L.IOU_CASES + L.IOU_BWD_ONLY:
        assert 2 * c["N"] < 2 ** 23 and c["N"] % 8 == 0 and c["why"], L.iou_id(c)
    for c in (L.IOU_ONES[1], L.IOU_TILED[4]):
        d = L.iou_exact_data(c)
        S = d["S"]
        assert S.dtype == np.float64 and np.array_equal(2 * S, np.round(2 * S)) and 2 * S.max() < 2 ** 23
        assert float(S[:, -1, -1].max()) == 0.0
        y = d["y"]
        assert (y[:, 0] == 0).all() and (y[:, -1] == 1).all(), "one all-zero and one all-one slot"
        assert set(np.unique(d["logits"]).tolist()) == set(L.EXACT_LOGITS)
        g = d["dlogits"]                                          # (small integer) * (1/4 or 0): exact in fp32
        assert np.array_equal(4 * g, np.round(4 * g)) and np.abs(g).max() <= 0.75 and np.abs(g).max() > 0
        T, G = c["T"], c["G"]
        perm = d["perm"]
        assert perm.shape[1] > T and perm.min() >= 0 and perm.max() < G
        for b in range(c["B"]):
            assert len(set(perm[b, :min(T, G)].tolist())) == min(T, G)


def test_quantised_scores_are_exact_in_float64():
    for G, T in L.ASSIGN_SIZES:
        assert 1 <= T <= G <= 128
        for st in L.ASSIGN_STRUCTS:
            s = L.assign_scores(G, T, st)
            assert s.shape == (L.ASSIGN_B, G, T) and s.dtype == F32 and np.isfinite(s).all()
            k = s.astype(np.float64) * L.Q20
            assert np.array_equal(k, np.round(k)) and s.min() >= 0 and s.max() < 16
            assert 128 * 16 * L.Q20 < 2 ** 53                    # any total of <= 128 entries, and the fp64 potentials, are exact
            if st == "train":
                assert (s[0][:, max(1, T - T // 4):] == 1.0).all() and (s[2] == 10.0).all() and (s[0] == 1.0).mean() >= 0.3
                n_inst = T // 2
                assert (s[1][n_inst:] == 10.0).all() and (s[1][:, n_inst:] == 10.0).all()
            if st == "dup" and G >= 2 and T >= 2:
                assert np.array_equal(s[:, 0], s[:, 1]) and np.array_equal(s[:, :, 0], s[:, :, 1])
            if G <= 20 or (G, T, st) in ((65, 65, "dup"), (100, 64, "train")):
                p = L.assign_sequential(s)                        # the sequential form of the kernels' algorithm is optimal, ties or not
                assert np.array_equal(L.assign_total(s, p), L.assign_optimum(s)) and not p[:, T:].any(), (G, T, st)
                assert all(len(set(p[b, :T].tolist())) == T for b in range(L.ASSIGN_B))
    assert L.assign_sequential(np.full((1, 3, 2), 0.5, F32)).tolist() == [[0, 1, 0]], "a constant matrix: the first free slot each time"
    # the optimum of a tiny matrix by hand, and a total
    s = np.array([[[0.5, 0.25], [0.25, 1.0], [1.0, 1.0]]], F32)
    assert L.assign_optimum(s).tolist() == [0.5] and L.assign_total(s, np.array([[1, 0, 0]])).tolist() == [0.5]


def test_heads_exact_cases_stay_below_2_to_24():
    """integer features / weights / gradients and probs 1 / npow: every d-logit is a multiple of 1 / npow^2 and every sum of |terms|,
    prefill included, stays below 2^24 such steps"""
    for s in L.HEADS_BWD_EXACT:
        d = L.heads_exact_data(s)
        rows, Cs, ncls = s
        assert L.heads_fits(rows, sum(Cs), ncls), L.heads_id(s)
        assert L.heads_exact_bound(d) < 2 ** 24, (L.heads_id(s), L.heads_exact_bound(d))
        q = d["ref"]["dl"] * d["npow"] ** 2
        assert np.array_equal(q, np.round(q))
        assert all((np.abs(v) >= 1).all() for v in d["fill"].values()), "the prefill has no zero"
        assert np.array_equal(d["stop"], np.round(d["stop"])) and np.abs(d["stop"]).max() < 2 ** 24
    assert {s[2] for s in L.HEADS_BWD_EXACT} >= {1, 2, 4, 16, 64}
    assert max(sum(s[1]) for s in L.HEADS_SHAPES) == L.HEADS_MAXK


# ---------------------------------------------------------------- restated launch rules
def test_softiou_plans_are_what_the_case_comments_claim():
    """rsis_l_softiou_sums restated (sums_plan) against the `expect` fields of the case table.  A retuned rule in losses.hip fails here:
    update the restated rule AND the cases (each must still cross its edge)."""
    for c in L.IOU_CASES:
        plan = L.sums_plan(c["B"], c["T"], c["G"], c["N"])
        assert plan == c["expect"], (L.iou_id(c), plan)
        det = L.sums_plan(c["B"], c["T"], c["G"], c["N"], True)
        assert det["per"] == c["N"] and det.get("waves", det.get("pgroups")) == 1
    assert 392 == 12 * 32 + 8 and L.sums_plan(32, 10, 20, 224 * 224)["per"] == 392, "the bench batch's per_wave"
    assert {c["expect"]["nG"] for c in L.IOU_TILED} == {1, 2, 4} and {c["expect"]["tshift"] for c in L.IOU_TILED} == {0, 1, 2}
    assert any(c["expect"]["nT"] == 3 for c in L.IOU_TILED), "a wave that returns early"
    b = L.IOU_BWD_ONLY[0]
    n4 = b["B"] * b["T"] * b["N"] // 4
    assert L.IOU_BWD_GRID_CAP < n4 < 2 * L.IOU_BWD_GRID_CAP and (n4, L.IOU_BWD_GRID_CAP) == (2359296, 2097152)
    assert [L.iou_id(c) for c in L.IOU_CASES if c not in L.IOU_NORMAL] == ["b2_t1_g1_n8", "b2_t32_g1_n64", "b2_t1_g32_n64"], "exact regime only"
    assert {c["expect"]["kernel"] for c in L.IOU_NORMAL} == {"ones", "tiled"}


def test_heads_lds_rule():
    """2 rows (ncls + 1) + rows ceil(K / rows) floats <= 64 KB: at 21 classes and K = 248 the last row count that fits is 364"""
    Cs, ncls = L.HEADS_LIMIT
    K = sum(Cs)
    assert K == 248 and L.heads_max_rows(K, ncls) == (364, 365)
    assert L.heads_lds_floats(364, K, ncls) == 364 * 45 == 16380 and L.heads_lds_floats(365, K, ncls) == 16425 > L.LDS_FLOATS == 16384
    assert all(L.heads_fits(r, K, ncls) for r in range(1, 365)) and not any(L.heads_fits(r, K, ncls) for r in range(365, 800))
    assert 28 * 13 == 364 and not L.heads_fits(28 * 14, K, ncls) and L.heads_fits(14, K, ncls)
    for s in L.HEADS_SHAPES:
        assert L.heads_fits(s[0], sum(s[1]), s[2]), L.heads_id(s)
    assert [L.heads_id(s) for s in L.HEADS_NORMAL] == ["r320_k128+64+32+16+8_c21", "r97_k16+8_c33", "r64_k2048_c64", "r7_k100+3+9+1+50_c17"]


def test_side_key_roundtrip_and_order():
    """the Python restatement of rsis_side_key: decode(encode) is the identity by BITS, and the key order is the value order (larger value
    first, then the smaller pixel)"""
    v, p = L.KEY_VALUES, L.KEY_PIXELS
    k = L.side_key(v, p)
    v2, p2 = L.side_key_decode(k)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(p2, p) and (k > 0).all()
    assert int(L.side_key(F32(0.0), 0)) == (0x80000000 << 32) | 0x7FFFFFFF and int(L.side_key(F32(-0.0), 0)) == (0x7FFFFFFF << 32) | 0x7FFFFFFF
    order = np.array([-L.F32_MAX, -1.5, -1e-40, -0.0, 0.0, 1e-40, 2.0 ** -126, 1.0, L.F32_MAX], F32)
    ks = L.side_key(order, 5)
    assert (ks[1:] > ks[:-1]).all()
    assert L.side_key(F32(1.0), 0) > L.side_key(F32(1.0), 1)
    d = L.keys_data()
    assert sum(np.isin(d["vals"][0].view(np.uint32), L.KEY_VALUES.view(np.uint32)).sum(1) >= len(L.KEY_VALUES)) == L.KEYS_SHAPE[0]
    sv = np.concatenate(d["vals"], 1).astype(np.float64)
    assert np.isfinite(np.abs(sv) @ np.abs(d["Ws"]).astype(np.float64)).all() and (np.abs(sv) @ np.abs(d["Ws"])).max() < 1e38


# ---------------------------------------------------------------- host models against brute-force loops
def test_sums_chain_against_a_loop():
    c = L._iou(2, 3, 2, 24, "tiny")
    rs = np.random.default_rng(3)
    logits, y = rs.normal(0, 2, (2, 3, 24)).astype(F32), (rs.random((2, 2, 24)) < 0.5).astype(F32)
    got = L.sums_chain32(logits, y)
    p = L.sigmoid32(logits)
    for b in range(2):
        for t in range(4):
            for g in range(3):
                acc = F32(0)
                for n in range(24):
                    a = p[b, t, n] if t < 3 else F32(1)
                    v = y[b, g, n] if g < 2 else F32(1)
                    acc = F32(acc + F32(a * v))
                want = acc if not (t == 3 and g == 2) else F32(0)
                assert got[b, t, g] == want, (b, t, g)
    S = L.sums64(L.sigmoid64(logits), y)
    assert 0 < np.abs(got - S).max() < 1e-5
    # one fp32 sigmoid by hand
    x = F32(0.75)
    assert L.sigmoid32(x) == F32(F32(1) / F32(F32(1) + np.exp(F32(-x), dtype=F32)))


def test_heads_host_model_against_a_loop():
    s = (3, [4, 2], 5)
    d = L.heads_normal_data(s, "normal")
    sv = np.concatenate(d["sides"], 1)
    for i in range(3):
        lg = []
        for r in range(6):
            w = d["Wc"][r] if r < 5 else d["Ws"]
            acc = F32(0)
            for k in range(6):
                acc = F32(acc + F32(sv[i, k] * w[k]))
            lg.append(F32(acc + (d["bc"][r] if r < 5 else d["bs"][0])))
        assert d["host"]["stop"][i] == lg[5]
        m = max(lg[:5])
        e = [np.exp(F32(v - m), dtype=F32) for v in lg[:5]]
        z = F32(0)
        for v in e:
            z = F32(z + v)
        assert [F32(v / z) for v in e] == d["host"]["probs"][i].tolist()
    # parameter gradient: a chain over the rows
    p, g = d["probs_in"], d["dprobs"]
    for r in (0, 4):
        for k in (0, 5):
            acc = F32(0)
            for i in range(3):
                dot = F32(0)
                for c in range(5):
                    dot = F32(dot + F32(g[i, c] * p[i, c]))
                acc = F32(acc + F32(F32(p[i, r] * F32(g[i, r] - dot)) * sv[i, k]))
            assert d["host"]["dW"][r, k] == acc
    assert np.abs(d["probs"].sum(1) - 1).max() < 1e-12


def test_tail_host_model_against_a_loop():
    c = dict(n=30, C=21, bw=False, cw=True, regime="normal", gout=True)
    q = L.tail_inputs(c)
    h = L.tail_eval(q, F32)
    w_iou, w_cls, w_stop = L.TAIL_W
    a_iou = a_cls = a_stop = F32(0)
    sum_m, sum_c = F32(q["swm"].sum()), F32(q["swc"].sum())
    bw = F32(sum_m / F32(30))
    for i in range(30):
        p, t, x = q["probs"][i, q["y"][i]], q["swm"][i], q["stop"][i]
        nll = F32(-np.log(p, dtype=F32) * q["cw"][q["y"][i]])
        mx = max(F32(-x), F32(0))
        lv = F32(F32(F32(x - F32(x * t)) + mx) + np.log(F32(np.exp(F32(-mx), dtype=F32) + np.exp(F32(F32(-x) - mx), dtype=F32)), dtype=F32))
        bal = F32(F32(F32(F32(1) - bw) * t) + F32(bw * F32(F32(1) - t)))
        if q["swm"][i] > 0:
            a_iou, a_cls = F32(a_iou + q["siou"][i]), F32(a_cls + nll)
        if q["swc"][i] > 0:
            a_stop = F32(a_stop + F32(lv * bal))
    l_iou, l_cls, l_stop = F32(a_iou / sum_m), F32(a_cls / sum_m), F32(a_stop / sum_c)
    total = F32(F32(F32(w_iou * l_iou) + F32(w_cls * l_cls)) + F32(w_stop * l_stop))
    assert h["out"].tolist() == [total, l_iou, l_stop, l_cls]
    r = L.tail_eval(q, np.float64)
    assert 0 < np.abs(h["out"] - r["out"]).max() < 1e-5
    # the reference is the oracle's arithmetic: MaskedNLL / StableBalancedMaskedBCE + masked means (train.py:159-176)
    import torch
    from oracle import rsis_oracle as O
    tt = lambda a: torch.from_numpy(np.asarray(a)).double()
    leaves = [tt(q[k]).requires_grad_() for k in ("probs", "stop", "siou")]
    nll = O.MaskedNLL(torch.from_numpy(q["y"]).reshape(-1, 1), leaves[0], tt(q["cw"]))
    bce = O.StableBalancedMaskedBCE(tt(q["swm"]), leaves[1], None)
    mm = lambda v, w: torch.masked_select(v.reshape(-1), torch.from_numpy(w > 0)).mean()
    parts = [mm(leaves[2], q["swm"]), mm(bce, q["swc"]), mm(nll, q["swm"])]
    ref = float(w_iou) * parts[0] + float(w_cls) * parts[2] + float(w_stop) * parts[1]
    (ref * float(L.TAIL_GOUT)).backward()
    assert np.allclose(r["out"], [float(ref.detach())] + [float(v.detach()) for v in parts], rtol=1e-13, atol=0)
    for k, leaf in zip(("dprobs", "dstop", "dsiou"), leaves):
        assert np.allclose(r[k], leaf.grad.numpy(), rtol=1e-12, atol=1e-300), k


# ---------------------------------------------------------------- every normal case has a yardstick
@pytest.mark.parametrize("regime", list(L.IOU_REGIMES))
def test_softiou_err_host_is_nonzero_and_finite(regime):
    for c in L.IOU_NORMAL:
        if c["N"] > 100000:
            continue                                             # the two large maps: test_largest_references_are_cheap
        d = L.iou_normal_data(c, regime)
        assert np.isfinite(d["err_host"]) and 0 < d["err_host"] < 1e-3 * c["N"], (L.iou_id(c), d["err_host"])
        assert np.isfinite(d["cost"]).all() and d["cost"].min() >= 0 and d["cost"].max() <= 1 and d["den"].min() > 0.5
    if regime == "hot":
        frac = float((np.abs(d["logits"]) > 10).mean())
        assert frac > 0.35, "most pixels of the hot regime are far into the sigmoid's tails: %.2f" % frac
        p = L.sigmoid32(d["logits"])
        assert (p == 0).any() or (p == 1).any()


@pytest.mark.parametrize("regime", ["normal", "hot"])
def test_heads_err_host_is_nonzero_and_finite(regime):
    for s in L.HEADS_NORMAL:
        d = L.heads_normal_data(s, regime)
        for k, v in d["err_host"].items():
            assert np.isfinite(v) and 0 < v < 1e-2, (L.heads_id(s), k, v)
        if regime == "hot":
            top = np.sort(d["probs"], 1)
            assert np.median(top[:, -1]) > 1 - 1e-7 and np.median(top[:, 0]) < 1e-14
            lg = np.log(np.maximum(top[:, -1], 1e-300)) - np.log(np.maximum(top[:, 0], 1e-300))
            assert np.median(lg) >= 30, "logit spread of the hot variant"


def test_tail_cases_have_a_yardstick_and_cover_the_table():
    assert {c["n"] for c in L.TAIL_CASES} == set(L.TAIL_N) and {c["C"] for c in L.TAIL_CASES} == {2, 21, 64}
    for n in L.TAIL_N:
        assert {c["regime"] for c in L.TAIL_CASES if c["n"] == n} == {"normal", "hot"}
    assert len({L.tail_id(c) for c in L.TAIL_CASES}) == len(L.TAIL_CASES)
    assert sum(1 for c in L.TAIL_CASES if c["n"] == 320 and c["regime"] == "normal") == 12 and any(not c["gout"] for c in L.TAIL_CASES)
    for c in L.TAIL_CASES:
        q = L.tail_inputs(c)
        r, h = L.tail_eval(q, np.float64), L.tail_eval(q, F32)
        err = float(np.abs(h["out"].astype(np.float64) - r["out"]).max())
        assert np.isfinite(r["out"]).all() and np.isfinite(err) and 0 < err < 1e-3, (L.tail_id(c), err)
        for k in ("dprobs", "dstop", "dsiou"):
            assert np.isfinite(r[k]).all(), (L.tail_id(c), k)
        assert q["swm"][0] == 1 and q["swc"][0] == 1
        bw = L.tail_auto_bw(q)
        assert bw <= L.TAIL_MAX_AUTO_BW or bw == 1.0, (L.tail_id(c), bw)        # the premise of K_DSTOP's count for 1 - bw
        if c["regime"] == "hot":
            pt = q["probs"][np.arange(c["n"]), q["y"]][q["swm"] > 0]
            assert pt.min() == F32(1e-30) and (c["n"] < 2 or (pt == 1.0).any())
            assert c["n"] < 30 or np.abs(q["stop"]).max() > 30
    assert float(L.TAIL_GOUT) != 1.0


# ---------------------------------------------------------------- cost
def test_largest_references_are_cheap():
    """the float64 references and host models of the largest soft-IoU cases, each under 5 s"""
    for c in (L.IOU_ONES[-1], L.IOU_ONES[-2], L.IOU_BWD_ONLY[0]):
        t0 = time.perf_counter()
        if c in L.IOU_BWD_ONLY:
            d = L.iou_exact_data(c, with_sums=False)
        else:
            d = L.iou_normal_data(c, "hot")
            assert np.isfinite(d["err_host"]) and d["err_host"] > 0
            L.iou_exact_data(c)
        dt = time.perf_counter() - t0
        print("%s: references and host model %.2f s" % (L.iou_id(c), dt))
        assert dt < 5.0, (L.iou_id(c), dt)
    t0 = time.perf_counter()
    L.heads_normal_data(L.HEADS_SHAPES[4], "hot")
    L.assign_optimum(L.assign_scores(128, 128, "train"))
    assert time.perf_counter() - t0 < 5.0
