"""Host-side checks of the fp32 resize / pooling tests (no GPU): every case of resample_cases.py takes the launch path its table entry
claims under the restated rules, every kernel, instantiation and index mode is reached, the restated rules still read like
rsis_amd/csrc/pointwise.hip, the float64 model of the resize agrees with F.interpolate to the coordinate error, a numpy emulation of
upsample_bwd_kernel's per-block tables gives the model's weights and stays inside its staged region, and the tie data has ties."""
import os
import re
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STALE = "the launch rules of rsis_amd/csrc/pointwise.hip changed: update the restated rule in tests/resample_cases.py and the cases at its edges"


def _src(name):
    with open(os.path.join(ROOT, "rsis_amd", "csrc", name)) as f:
        return re.sub(r"\s+", " ", f.read())


# ---------------------------------------------------------------- the rules still read like the source
RULE_TEXT = {
    "pointwise.hip": [
        "Ho >= 16 && Wo >= 128 && fh * 15 + 3.f <= 12 && fw * 127 + 6.f <= 72",
        "Ho >= 32 && Wo >= 64 && fh * 31 + 3.f <= 20 && fw * 63 + 6.f <= 48",
        "const bool al = Wo % 4 == 0 && Wi % 4 == 0;",
        "upsample_fwd_lds_kernel<16, 128, 12, 18>", "upsample_fwd_lds_kernel<32, 64, 20, 12>",
        "if (Wq <= 256 && (Wq & (Wq - 1)) == 0) { shift = 0; while ((1 << shift) < Wq) ++shift; } if (shift < 0 && Wq <= 256) shift = -2;",
        "#define UK 6",
        "const bool tiled = smin > 0.f && (2.f / smin + 1.f <= UK);",
        "const int ut = (Hi > 16 || Wi > 16) ? 32 : 16;",
        "const bool fits = tiled && ((ut - 1) / smin + UK + 3 <= (ut == 32 ? 80 : 44));",
        "long ppb = BC * tiles_x * tiles_y / 2048; if (ppb < 1) ppb = 1; if (ppb > 16) ppb = 16;",
        "const int vec = Wo % 4 == 0;",
        "upsample_bwd_kernel<32, 80>", "upsample_bwd_kernel<16, 44>",
        "int l = max(0, (int)floorf((i - 1) / sc) - 1);", "o < out && o < l + 4 + UK", "if (first < 0) first = min(l, out - 1);",
        "ext[tid] = min(min(last, out - 1) - o0 + 1, RM);",
        "reg[min(max(r0 + k, 0), ey - 1) * RP + cs + c]", "tmp[ly * RP + min(max(c0 + k, 0), ex - 1)]",
        "if ((H & 1) == 0 && (W & 3) == 0) { hipLaunchKernelGGL(maxpool3x3s2_bwd_v8_kernel",
        "if ((HW & 3) == 0) { // float4 loads, 8 in flight per thread",
        "for (int g0 = threadIdx.x; g0 < n4; g0 += 256 * 8)",
    ],
    "common.h": [
        "long g = (total + 255) / 256; if (g > 256 * 16) g = 256 * 16; if (g < 1) g = 1;",
        "return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;",
        "const float src = scale * of; i0 = (int)src; if (i0 > in - 1) i0 = in - 1; i1 = i0 + (i0 < in - 1 ? 1 : 0); l1 = fmaf(scale, of, -(float)i0);",
    ],
}


@pytest.mark.parametrize("name", sorted(RULE_TEXT))
def test_restated_rules_still_read_like_the_source(name):
    text = _src(name)
    for line in RULE_TEXT[name]:
        assert line in text, "%s\n  (no longer in %s: `%s`)" % (STALE, name, line)


# ---------------------------------------------------------------- every case takes the path it claims
@pytest.mark.parametrize("c", R.UP_FWD, ids=R.case_id)
def test_forward_case_takes_its_path(c):
    assert c["why"]
    got = R.upsample_fwd_path(c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"])
    assert got == c["path"], "%s: the rule gives %s, the table says %s.  %s" % (R.case_id(c), got, c["path"], STALE)
    # no case sits within rounding of a gate: float64 arithmetic (and a fused multiply-add on the host) decides the same way
    for which in R.LDS_TILES:
        t = R.LDS_TILES[which]
        if c["Ho"] >= t["toh"] and c["Wo"] >= t["tow"]:
            assert all(abs(s) > R.ROBUST for s in R.lds_gate_sides(which, c["Hi"], c["Wi"], c["Ho"], c["Wo"], np.float64)), which
    assert c["BC"] * c["Ho"] * c["Wo"] * 4 <= 11 << 20


@pytest.mark.parametrize("c", R.UP_BWD, ids=R.case_id)
def test_backward_case_takes_its_path(c):
    assert c["why"]
    p = R.upsample_bwd_path(c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"])
    assert p["kernel"] == c["path"], "%s: the rule gives %s, the table says %s.  %s" % (R.case_id(c), p["kernel"], c["path"], STALE)
    for k in ("ppb", "vec"):
        if k in c:
            assert p[k] == c[k], "%s: %s = %d, the table says %d.  %s" % (R.case_id(c), k, p[k], c[k], STALE)
    smin = min(float(c["Hi"] - 1) / (c["Ho"] - 1), float(c["Wi"] - 1) / (c["Wo"] - 1))
    if smin > 0 and not c.get("on_gate"):
        ut = 32 if max(c["Hi"], c["Wi"]) > 16 else 16
        assert abs(2 / smin + 1 - R.UK) > R.ROBUST and abs((ut - 1) / smin + R.UK + 3 - (80 if ut == 32 else 44)) > R.ROBUST
    assert c["BC"] * max(c["Ho"] * c["Wo"], c["Hi"] * c["Wi"]) * 4 <= 11 << 20


def test_every_forward_kernel_and_index_mode_is_reached():
    paths = {c["path"] for c in R.UP_FWD}
    assert paths >= {"lds16x128", "lds32x64", "scalar", "v4[0]", "v4[3]", "v4[8]", "v4[-2]", "v4[-1]"}, STALE
    by = lambda p: [c for c in R.UP_FWD if c["path"] == p]
    for which in R.LDS_TILES:
        t = R.LDS_TILES[which]
        cs = by(which)
        assert any(c["Ho"] == t["toh"] and c["Wo"] == t["tow"] for c in cs), "one tile"
        assert any(c["Ho"] % t["toh"] and c["Wo"] % t["tow"] and c["Ho"] > t["toh"] and c["Wo"] > t["tow"] for c in cs), "partial tiles both ways"
        assert any(w % 4 == 3 for c in cs for (_, ow0, _, w) in R.lds_tile_origins(which, c["Hi"], c["Wi"], c["Ho"], c["Wo"]) if ow0), "w_lo % 4 == 3"
    # the tail block of the wq_shift >= 0 mode, the one live thread of the second blockIdx.y block, both second trips
    assert any(c["path"] == "v4[3]" and (c["BC"] * c["Ho"]) % 32 for c in R.UP_FWD)
    assert any(c["path"] == "v4[0]" and (c["BC"] * c["Ho"]) % 256 and c["BC"] * c["Ho"] > 256 for c in R.UP_FWD)
    assert any(c["path"] == "v4[-1]" and c["Wo"] // 4 == 257 for c in R.UP_FWD)
    assert any(c["path"] == "scalar" and c["BC"] * c["Ho"] * c["Wo"] > R.TWO20 for c in R.UP_FWD)
    assert sum(1 for c in R.UP_FWD if c.get("identity")) >= 2
    # each gate is failed by its smallest step, from a case that passes
    for which in R.LDS_TILES:
        Hi, Wi, Ho, Wo = R.find_fwd_gate_edge(which)
        assert R.upsample_fwd_path(2, Hi, Wi, Ho, Wo) == which
        assert R.lds_gate_sides(which, Hi + 1, Wi, Ho, Wo)[0] > 0 and R.lds_gate_sides(which, Hi, Wi + 4, Ho, Wo)[1] > 0
        print("%s gate edge: (%d, %d) -> (%d, %d), fh %.4f fw %.4f" % (which, Hi, Wi, Ho, Wo, R.ac_scale(Hi, Ho), R.ac_scale(Wi, Wo)))


def test_every_backward_kernel_and_mode_is_reached():
    ps = [(c, R.upsample_bwd_path(c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"])) for c in R.UP_BWD]
    tiled = [(c, p) for c, p in ps if p["kernel"] != "generic"]
    for ut in (16, 32):
        mine = [(c, p) for c, p in tiled if p["ut"] == ut]
        assert {p["vec"] for _, p in mine} == {0, 1}, "vec and scalar staging, ut = %d" % ut
        n, fit, nofit = R.find_bwd_fit_edge(ut)
        assert any(c["Hi"] == n and c["Ho"] == fit for c, _ in mine) and any(c["Hi"] == n and c["Ho"] == nofit and p["kernel"] == "generic" for c, p in ps)
        print("ut = %d fit edge: %d -> %d tiled (scale %.4f), -> %d generic" % (ut, n, fit, R.ac_scale(n, fit), nofit))
    assert any(p["ut"] == 32 and min(c["Hi"], c["Wi"]) <= 16 for c, p in tiled)
    assert any(p["tiles_x"] > 1 and p["tiles_y"] > 1 and c["Hi"] % 32 and c["Wi"] % 32 for c, p in tiled)
    assert any(p["ppb"] == 2 and c["BC"] % 2 for c, p in tiled) and any(p["ppb"] == 16 and c["BC"] % 16 for c, p in tiled)
    assert any(p["ppb"] > 1 and p["tiles_x"] * p["tiles_y"] > 1 for c, p in tiled)
    assert any(c["Hi"] > 2 * c["Ho"] for c, p in tiled), "the tiled kernel down-sampling"
    gen = [(c, p) for c, p in ps if p["kernel"] == "generic"]
    assert any(p["items"] > R.TWO20 and p["grid"] == R.GRID_CAP for c, p in gen)
    assert any(0 < R.ac_scale(c["Wi"], c["Wo"]) < 0.25 for c, p in gen) and any(R.ac_scale(c["Hi"], c["Ho"]) > 2 for c, p in gen)
    # pool_arg reaches pixel 0, the last pixel, a tile's last row and column and the first pixel of the second tile
    c = next(c for c, p in tiled if p["tiles_x"] > 1)
    a = set(R.pool_args(c).tolist())
    assert {0, c["Hi"] * c["Wi"] - 1, (min(32, c["Hi"]) - 1) * c["Wi"] + 31, 32} <= a


def test_pool_cases_take_their_paths():
    assert R.ew_grid(1) == 1 and R.ew_grid(R.TWO20) == R.GRID_CAP and R.ew_grid(1 << 30) == R.GRID_CAP and R.ew_grid(257) == 2
    assert {(c["path"], c["trips"]) for c in R.GMAX_FWD} >= {("vector", 1), ("vector", 2), ("scalar", 1), ("scalar", 6)}, STALE
    for c in R.GMAX_FWD:
        assert c["path"] == ("vector" if c["HW"] % 4 == 0 else "scalar") and c["why"]
    assert {c["kind"] for c in R.GMAX_FWD} == {"cont", "ties", "edges"}
    assert R.GMAX_BWD_BIG["BC"] * R.GMAX_BWD_BIG["HW"] > R.TWO20 and R.GMAX_BWD_ADD["BC"] % 256
    for c in R.MAXPOOL:
        assert c["path"] == R.maxpool_bwd_path(c["H"], c["W"]) and c["why"]
    for path in ("v8", "scalar"):
        assert any(c["path"] == path and c["items"] > R.TWO20 for c in R.MAXPOOL), path
    assert any(c["BC"] * R.pool_out(c["H"]) * R.pool_out(c["W"]) > R.TWO20 for c in R.MAXPOOL), "forward second trip"
    assert any(c["H"] == 1 and c["W"] > 1 for c in R.MAXPOOL) and any(c["W"] == 1 and c["H"] > 1 for c in R.MAXPOOL)
    old = [(8, 8, 8), (15, 9, 11), (2, 16, 6), (6, 7, 7), (6, 12, 20), (2, 10, 4), (16, 32, 64)]            # test_maxpool3x3s2's shapes
    assert all(any((c["BC"], c["H"], c["W"]) == o for c in R.MAXPOOL) for o in old)


# ---------------------------------------------------------------- the LDS kernels' staged patch covers every read
@pytest.mark.parametrize("c", [c for c in R.UP_FWD if c["path"] in R.LDS_TILES], ids=R.case_id)
def test_lds_patch_covers_every_source_pixel(c):
    t = R.LDS_TILES[c["path"]]
    Hi, Wi, Ho, Wo = c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    fh, fw = R.ac_scale(Hi, Ho), R.ac_scale(Wi, Wo)
    worst_r = worst_c = 0
    for oh0, ow0, h_lo, w_lo in R.lds_tile_origins(c["path"], Hi, Wi, Ho, Wo):
        h1 = R.ac_coord(np.arange(oh0, min(oh0 + t["toh"], Ho)), fh, Hi)[1]
        w1 = R.ac_coord(np.arange(ow0, min(ow0 + t["tow"], Wo)), fw, Wi)[1]
        worst_r, worst_c = max(worst_r, int(h1.max()) - h_lo), max(worst_c, int(w1.max()) - (w_lo & ~3))
    assert worst_r < t["rh"] and worst_c < t["rq"] * 4, "rows %d of %d, columns %d of %d" % (worst_r + 1, t["rh"], worst_c + 1, t["rq"] * 4)
    print("%s: %d of %d staged rows, %d of %d staged columns used" % (R.case_id(c), worst_r + 1, t["rh"], worst_c + 1, t["rq"] * 4))
    if (Hi, Wi, Ho, Wo) == R.find_fwd_gate_edge(c["path"]):
        # a tile's rows span int(fh (oh0 + TOH - 1)) + 1 - int(fh oh0) <= floor(fh (TOH - 1)) + 2 source rows, and the gate keeps
        # fh (TOH - 1) <= RH - 3: RH - 1 rows is the most any admitted size reads (the last staged row is spare), and this case reads them
        assert worst_r + 1 == t["rh"] - 1


# ---------------------------------------------------------------- resize_matrices against F.interpolate
@pytest.mark.parametrize("dims", sorted({(c["Hi"], c["Ho"], c["Wi"], c["Wo"]) for c in R.UP_FWD + R.UP_BWD}))
def test_resize_matrices_against_interpolate(dims):
    Hi, Ho, Wi, Wo = dims
    Ah, Aw = R.resize_matrices(Hi, Ho, Wi, Wo)
    for A in (Ah, Aw):
        assert np.abs(A.sum(1) - 1).max() <= 2.0 ** -23
        assert (A != 0).sum(1).max() <= 2 and A.min() >= -R.coord_delta(A.shape[1]) and A.max() <= 1 + R.coord_delta(A.shape[1])
    x = np.random.default_rng(Hi * 1000 + Wo).normal(0, 1, (2, Hi, Wi))
    ref = F.interpolate(torch.from_numpy(x)[None], size=(Ho, Wo), mode="bilinear", align_corners=True)[0].numpy()
    slope_h = np.abs(np.diff(x, axis=1)).max() if Hi > 1 else 0.0
    slope_w = np.abs(np.diff(x, axis=2)).max() if Wi > 1 else 0.0
    bar = R.coord_delta(Hi) * slope_h + R.coord_delta(Wi) * slope_w + 4 * 2.0 ** -53 * np.abs(x).max()
    err = np.abs(Ah @ x @ Aw.T - ref).max()
    assert err <= bar, "model vs F.interpolate: %.3e, the coordinate error allows %.3e" % (err, bar)


def test_fused_and_rounded_coordinates_differ_by_more_than_the_model_bar():
    """why ac_coord spells its fused multiply-add out: with l1 = fl(scale * o) - i0 (two roundings) in one kernel and the fused form in
    another, the two differ by up to half an ulp of the coordinate -- several times the 8u bar of the forward model on a 128-wide map"""
    c = next(c for c in R.UP_FWD if c["Wo"] == 310)
    Wi, Wo = c["Wi"], c["Wo"]
    sc = R.ac_scale(Wi, Wo)
    i0, _, l1 = R.ac_coord(np.arange(Wo), sc, Wi)
    l1_rounded = (sc * np.arange(Wo).astype(np.float32)) - i0.astype(np.float32)
    worst = np.abs(l1.astype(np.float64) - l1_rounded.astype(np.float64)).max()
    print("max |fused l1 - rounded l1| = %.3e = %.1f u at Wi = %d" % (worst, worst / R.U, Wi))
    assert 8 * R.U < worst <= 2.0 ** -24 * Wi


# ---------------------------------------------------------------- upsample_bwd_kernel's tables, emulated
TILED = [c for c in R.UP_BWD if c["path"].startswith("tiled")]
AXES = sorted({(n_in, n_out, int(c["path"][5:])) for c in TILED for n_in, n_out in ((c["Hi"], c["Ho"]), (c["Wi"], c["Wo"]))})


@pytest.mark.parametrize("axis", AXES, ids=lambda a: "%d_to_%d_ut%d" % a)
def test_tiled_backward_tables_give_the_model_weights_inside_the_region(axis):
    n_in, n_out, ut = axis
    W, bad = R.bwd_axis_effective(n_in, n_out, ut, 80 if ut == 32 else 44)
    assert not bad, "region index outside [0, ext) for input indices inside the map: (input, k, index) %s" % bad[:8]
    A = R.axis_matrix(n_in, n_out)
    i0, i1, _ = R.ac_coord(np.arange(n_out), R.ac_scale(n_in, n_out), n_in)
    tol = np.zeros_like(A)
    tol[np.arange(n_out)[i0 == i1], i0[i0 == i1]] = 2.0 ** -24        # (1 - l1) + l1 at the clamped last index: summed in fp32 by the kernel
    assert (np.abs(W.T - A) <= tol).all(), "the tables' weights differ from the forward's by up to %.3e" % np.abs(W.T - A).max()


def test_down_sampling_read_above_the_region_before_the_clamp():
    """the index rule of the parent commit, min(r0 + k, ext - 1) alone, reads LDS at a negative index at 40 -> 17"""
    W, bad = R.bwd_axis_effective(40, 17, 32, 80, clamp0=False)
    print("40 -> 17, ut 32, without the clamp at 0: (input index, k, region index) %s" % bad)
    assert bad and all(idx < 0 for _, _, idx in bad)
    assert not R.bwd_axis_effective(40, 17, 32, 80, clamp0=True)[1]
    # up-sampling never needed the clamp
    for n_in, n_out, ut in AXES:
        if n_out >= n_in:
            assert not R.bwd_axis_effective(n_in, n_out, ut, 80 if ut == 32 else 44, clamp0=False)[1]


# ---------------------------------------------------------------- the references are cheap, the tie data has ties
def test_largest_reference_is_cheap():
    t0 = time.perf_counter()
    big_f = max(R.UP_FWD, key=lambda c: c["BC"] * c["Ho"] * c["Wo"])
    R.up_fwd_refs(big_f)
    t_f = time.perf_counter() - t0
    big_b = max(R.UP_BWD, key=lambda c: c["BC"] * c["Ho"] * c["Wo"])
    R.up_bwd_refs(big_b)
    t_b = time.perf_counter() - t0 - t_f
    big_m = max(R.MAXPOOL, key=lambda c: c["BC"] * c["H"] * c["W"])
    x, dy, _ = R.maxpool_data(big_m, True)
    R.maxpool_ref(x, dy)
    t_m = time.perf_counter() - t0 - t_f - t_b
    print("float64 references: forward %s %.2f s, backward %s %.2f s, 3x3 pool %s %.2f s" % (R.case_id(big_f), t_f, R.case_id(big_b), t_b, R.case_id(big_m), t_m))
    assert t_f < 5.0 and t_b < 5.0 and t_m < 8.0


@pytest.mark.parametrize("c", R.GMAX_FWD, ids=R.case_id)
def test_global_pool_data_and_reference(c):
    x = R.gmax_data(c)
    v, a = R.gmax_ref(x)
    assert np.array_equal(a, np.argmax(x, axis=1)) and np.array_equal(v, x.max(1).astype(np.float64))      # the FIRST maximum; 0 for all -inf
    HW = c["HW"]
    if c["kind"] == "ties" and HW > 1:
        firsts, multi = set(), 0
        for j in range(c["BC"]):
            at = np.flatnonzero(x[j] == x[j].max())
            owners = {R.gmax_owner(int(i), HW) for i in at}
            assert len(at) >= 2 and len(owners) >= 2, "plane %d: the maxima lie in one thread's share" % j
            assert len({int(i) // 64 for i in at}) >= 2 or HW <= 64, "plane %d: the maxima lie in one 64-element share" % j
            if HW >= 1320:
                assert len({o // 64 for o in owners}) >= 2, "plane %d: the maxima lie in one wave's share" % j
            multi += any(R.gmax_owner(int(i), HW) == R.gmax_owner(int(at[0]), HW) for i in at[1:])
            firsts.add(int(at[0]) * 3 // HW)
        assert len(firsts) >= 2, "the first maximum sits in the same third of every plane"
        # the thread that owns the first maximum holds a later one as well (a scan that kept its LAST maximum would answer differently)
        assert multi >= (c["BC"] if HW >= 16384 else 1 if c["path"] == "vector" and HW >= 1320 else 0)
    if c["kind"] == "edges":
        assert np.isneginf(x[0]).all() and a[0] == 0 and a[1] == HW - 1 and a[2] == HW - 1 and a[3] == HW - 1
        assert (x[1, :-1] < x[1, -1]).all()


@pytest.mark.parametrize("c", R.MAXPOOL[:11], ids=R.case_id)
def test_window_pool_data_has_ties(c):
    x, dy, pre = R.maxpool_data(c, True)
    assert np.abs(dy).max() <= 3 and np.array_equal(dy, np.round(dy)) and np.array_equal(pre, np.round(pre))
    if c["H"] * c["W"] < 4:
        return
    cols = F.unfold(F.pad(torch.from_numpy(x)[:, None], (1, 1, 1, 1), value=float("-inf")), 3, stride=2)      # (BC, 9, windows)
    n_max = (cols == cols.max(1, keepdim=True).values).sum(1)
    assert int(n_max.max()) >= 2, "no window holds two equal maxima"
