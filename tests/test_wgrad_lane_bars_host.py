"""The bars of tests/test_gpu_wgrad_lanes.py must be able to fail (CPU only).  For every case of tests/wgrad_lane_cases.py four wrong
"results" are built from the float64 reference alone:
  (a) tile_left_out    one spatial tile of one image (64 pixels of the register-staged kernels, tw x w3t_th of the blk 3x3) is missing
                       from the sum;
  (b) split_twice      the tiles of one split at L = 2 are added twice;
  (c) taps_transposed  dW[co][ci][r][s] holds the sum of tap (s, r) (3x3 cases);
  (d) truncated        the operands are truncated to bf16, not rounded to nearest (bf16 / blk cases: an fp32 job rounds nothing).
TIGHT rejects (a)-(d) on every case, ROUNDING rejects (a)-(c) on every case, and the reference itself passes both with err = 0.  Also
here: the restated dispatch rule reaches every instantiation, and the lane-specific cases plan the launches they are named for."""
import pytest
import torch

import wgrad_lane_cases as LC


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_every_instantiation_has_a_case(family):
    """every register-staged (3, BM, TW, aligned or ragged) / (1, BM, BN, aligned or ragged) and every blk (3, BM, TW) / (1, BM, BN)
    instantiation is reached by a case of the family's grouped calls"""
    have = set().union(*[LC.instantiations(c) for c in LC.CALLS[family + "/all"]])
    assert have == set().union(*[LC.instantiations(c) for c in LC.CALLS[family + "/base"]]), "the instantiation list is `base`"
    want = LC.all_instantiations(family)
    assert len(want) == (26 if family == "bf16" else 13)
    assert want <= have, "no case for %r" % sorted(want - have)


def _plan(jobs):
    """wgb_plan_lanes of wgrad_lanes.h for one bucket in default mode, restated: jobs = [(dW tiles, spatial tiles)] -> per launch
    [(splits, tiles per split, items)] (the host walk of the real planner is tests/test_wgrad_lanes_host.py)"""
    total = sum(nt * sp for nt, sp in jobs)
    L = max(2, LC._cdiv(total, LC.WGB_TARGET))
    launches, cur, items = [], [], 0
    for nt, sp in jobs:
        nsplit = max(1, LC._cdiv(sp, L))
        tps = LC._cdiv(sp, nsplit)
        nsplit = LC._cdiv(sp, tps)
        nit = min(nsplit, 8)
        if len(cur) == LC.WGB_MAXJ or items + nit > 8 * LC.WGB_LANE_ITEMS:
            launches.append(cur)
            cur, items = [], 0
        cur.append((nsplit, tps, nit))
        items += nit
    return launches + [cur]


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_lane_cases_plan_the_launches_they_are_named_for(family):
    def bucket(call, key3):
        return [(LC.dw_tiles(c, j), LC.spatial_tiles(c, j)) for c in LC.CALLS[family + "/" + call] for j in c.jobs
                if LC.wgb_key(c, j)[:4] == key3]
    for call, key in (("splits", (3, 32, 32, 8)), ("splits", (1, 64, 64, 64))):
        (launch,) = _plan(bucket(call, key))
        assert launch == [(12, 2, 8)], launch                      # 23 tiles: 12 splits of 2, the last one a single tile, 8 items
    launches = _plan(bucket("many", (3, 32, 32, 8)))
    assert [len(l) for l in launches] == [32, 8] and set(launches[0]) == {(1, 1, 1)}
    launches = _plan(bucket("items", (3, 32, 32, 8)))
    assert [len(l) for l in launches] == [28, 1] and set(launches[0] + launches[1]) == {(8, 2, 8)}
    (launch,) = _plan(bucket("pad", (3, 32, 32, 8)))
    assert launch == [(1, 1, 1), (3, 2, 3)]                        # a one-block item next to three two-tile splits: padding blocks


def _rejects(c, got, bar):
    return LC.ratio(c, got, bar)[0] > 1.0


@pytest.mark.parametrize("call", [c for c in LC.CALLS if not c.endswith("/all")])      # (`all` holds the same cases again)
def test_bars_reject_wrong_results_and_pass_the_reference(call):
    for c in LC.CALLS[call]:
        R = LC.reference(c)
        for bar in LC.BARS:
            assert LC.ratio(c, R["ref"], bar)[0] == 0.0
            assert torch.isfinite(LC.BARS[bar](c, R)).all() and float(LC.BARS[bar](c, R).min()) > 0.0
        hows = [h for h in LC.WRONG if not (h == "taps_transposed" and c.ks != 3) and not (h == "truncated" and c.dtype == "f32")]
        for how in hows:
            got = LC.wrong_result(c, how)
            assert _rejects(c, got, "TIGHT"), "TIGHT passes %s on %r: err / bar %.3g" % (how, c, LC.ratio(c, got, "TIGHT")[0])
            if how != "truncated":
                assert _rejects(c, got, "ROUNDING"), "ROUNDING passes %s on %r: err / bar %.3g" % (how, c, LC.ratio(c, got, "ROUNDING")[0])


def test_mixed_call_holds_what_it_says():
    by = {c.name.split("/")[1]: c for c in LC.CALLS["mixed"]}
    assert LC.wgl_class(by["f32_staged5"], by["f32_staged5"].jobs[0]) == 5 and LC.wgl_class(by["f32_staged2"], by["f32_staged2"].jobs[0]) == 2
    assert LC.wgl_class(by["f32_tiled3"], by["f32_tiled3"].jobs[0]) == -1 and LC.wgl_class(by["f32_tiled1"], by["f32_tiled1"].jobs[0]) == 7
    assert len(LC.instantiations(by["bf16_1a"]) | LC.instantiations(by["bf16_1b"])) == 2
    assert len(LC.instantiations(by["bf16_3a"]) | LC.instantiations(by["bf16_3b"])) == 2
    assert by["f32_stride2"].stride == 2 and by["f32_cout1"].Cout == 1
