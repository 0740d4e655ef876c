"""--ignore_regions without a device: the flag, the C ABI declarations against the ctypes table, the float64 statement of the masked
soft-IoU sums against a per-pixel loop, and the numpy statements of the two map rules on hand-written arrays."""
import os
import re

import numpy as np

import ignore_map_cases as M
import loss_path_cases as L
import softiou_ignore_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _own_flag_sets():
    """argument lists built from the parser's OWN option table: every option once, valued options with their default (or first choice)
    in the `-name=value` form and again in the `-name value` form, every switch; then the training command lines the README gives"""
    from rsis_amd.args import _FLAGS
    eq, sp, switches = [], [], []
    for flag, kw in _FLAGS:
        if kw.get("action") in ("store_true", "store_false"):
            switches.append(flag)
            continue
        value = kw.get("default")
        if value is None:
            value = kw["choices"][0] if kw.get("choices") else (1 if kw.get("type") in (int, float) else "x")
        eq.append("%s=%s" % (flag, value))
        sp += [flag, str(value)]
    readme = ["--synthetic -batch_size 32 -maxseqlen 10 --use_class_loss --use_stop_loss --update_encoder --log_term -dtype bf16 --graph",
              "-dataset pascal -pascal_dir D --resize -model_name NAME",
              "-dataset cityscapes -cityscapes_dir D -num_classes 9 -maxseqlen 20 -gt_maxseqlen 20 --augment --curriculum_learning -model_name NAME"]
    return [eq, sp, [f for f in switches if f != "--ignore_regions"]] + [r.split() for r in readme]


def test_flag_parses_and_defaults_off():
    from rsis_amd.args import get_parser
    p = get_parser()
    assert p.parse_args([]).ignore_regions is False
    assert p.parse_args(["--ignore_regions"]).ignore_regions is True
    a = p.parse_args(["--synthetic", "--ignore_regions", "--log_term", "--graph", "-dtype", "bf16"])
    assert a.ignore_regions and a.synthetic and a.graph and a.dtype == "bf16"
    sets = _own_flag_sets()
    assert len(sets[0]) > 40 and len(sets[2]) > 15
    for flags in sets:                                   # every other flag set parses as before, with and without the new switch
        assert p.parse_args(flags).ignore_regions is False
        assert p.parse_args(flags + ["--ignore_regions"]).ignore_regions is True


def _declared(name):
    """the parameter list of `name` as include/rsis_hip.h declares it"""
    with open(os.path.join(ROOT, "include", "rsis_hip.h")) as f:
        text = f.read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, "%s is not declared in include/rsis_hip.h" % name
    return [p.strip() for p in m.group(1).split(",")]


def test_symbols_are_declared_and_bound_with_matching_arity():
    from rsis_amd._lib import SIGNATURES
    for name, plain in (("rsis_softiou_sums_ignore", "rsis_softiou_sums"), ("rsis_softiou_bwd_ignore", "rsis_softiou_bwd")):
        params = _declared(name)
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == len(params), name
        # the plain entry point's parameters plus the map, third
        assert len(params) == len(_declared(plain)) + 1 and "unsigned char" in params[2] and "ignore" in params[2]
        assert [p for k, p in enumerate(params) if k != 2] == _declared(plain)
    params = _declared("rsis_paint_ignore_map")
    assert "rsis_paint_ignore_map" in SIGNATURES and len(SIGNATURES["rsis_paint_ignore_map"][1]) == len(params) == 14


def test_float64_statement_against_a_pixel_loop():
    """2 x 3 x 4 x 16: I, P, Y summed pixel by pixel over the kept pixels; the cost of an image ignored everywhere is 1"""
    rs = np.random.default_rng(3)
    B, T, G, N = 2, 3, 4, 16
    logits = rs.normal(0, 2, (B, T, N)).astype(np.float32)
    y = (rs.random((B, G, N)) < 0.5).astype(np.float32)
    ign = np.where(rs.random((B, N)) < 0.4, rs.integers(1, 256, (B, N)), 0).astype(np.uint8)
    assert 0 < int((ign != 0).sum()) < B * N
    p = L.sigmoid64(logits)
    S = C.sums64_ignore(p, y, ign)
    for b in range(B):
        for t in range(T):
            for g in range(G):
                assert abs(S[b, t, g] - sum(p[b, t, n] * float(y[b, g, n]) for n in range(N) if ign[b, n] == 0)) < 1e-12
            assert abs(S[b, t, G] - sum(p[b, t, n] for n in range(N) if ign[b, n] == 0)) < 1e-12
        for g in range(G):
            assert S[b, T, g] == sum(float(y[b, g, n]) for n in range(N) if ign[b, n] == 0)
        assert S[b, T, G] == 0.0
    # the host model agrees with it to fp32 accuracy, and the gradient statement is zero exactly where the map is set
    assert np.abs(C.sums_chain32_ignore(logits, y, ign).astype(np.float64) - C.sums64_ignore(L.sigmoid64(logits), y, ign)).max() < 1e-5
    perm = np.tile(np.arange(G), (B, 1)).astype(np.int64)
    ca, cb = rs.normal(0, 1, (B, T)).astype(np.float32), rs.normal(0, 1, (B, T)).astype(np.float32)
    d = C.bwd64_ignore(logits, y, ign, perm, ca, cb)
    assert (d[np.broadcast_to((ign != 0)[:, None, :], d.shape)] == 0).all() and (d[np.broadcast_to((ign == 0)[:, None, :], d.shape)] != 0).all()
    ones = np.ones((B, N), np.uint8)
    cost, _den = L.cost64(C.sums64_ignore(p, y, ones))
    assert (cost == 1.0).all()


def test_cases_cover_both_families_and_pin_the_masking_of_y():
    for c in C.IGN_ONES:
        assert L.sums_plan(c["B"], c["T"], c["G"], c["N"])["kernel"] == "ones"
    for c in C.IGN_TILED:
        assert L.sums_plan(c["B"], c["T"], c["G"], c["N"])["kernel"] == "tiled"
    assert {L.sums_plan(c["B"], c["T"], c["G"], c["N"])["nG"] for c in C.IGN_TILED} == {1, 2, 4}
    c = C.IGN_BWD_ONLY[0]
    assert c["B"] * c["T"] * c["N"] // 4 > L.IOU_BWD_GRID_CAP and c["N"] == 1048576
    assert len(C.IGN_NORMAL) >= 6 and C.M_IOU_IGN <= 4.0
    for c in C.IGN_CASES:
        for pattern in C.PATTERNS:
            ign = C.ignore_map(c, pattern)
            assert ign.shape == (c["B"], c["N"]) and ign.dtype == np.uint8
            want = dict(zero=0, ones=c["B"] * c["N"], step=8 * c["B"], image=c["N"]).get(pattern)
            assert want is None or int((ign != 0).sum()) == want
            if pattern == "step":
                for b in range(c["B"]):
                    at = np.flatnonzero(ign[b])
                    assert at[0] % 8 == 0 and (np.diff(at) == 1).all()
        d = C.exact_data(c, "p30")
        assert int(d["ignore"].max()) > 1                                 # any non-zero byte ignores
        under = np.broadcast_to((d["ignore"] != 0)[:, None, :], d["y"].shape)
        assert (d["y"][under] == 1).all()                                  # ones under the map, in every slot: Y must be masked by the kernel
        assert (d["S"] != L.sums64(L.sigmoid32(d["logits"]), d["y"]))[:, c["T"], :c["G"]].all()


def test_cityscapes_rule_on_a_hand_written_map():
    from rsis_amd.dataloader.cityscapes import CLASS_OF_LABEL
    raw = np.array([[0, 7, 23, 24, 25, 26], [27, 28, 29, 30, 31, 32], [33, 34, 999, 1000, 24000, 26003], [29001, 33999, 255, 65535, 11, 1]])
    want = np.array([[0, 0, 0, 1, 1, 1], [1, 1, 0, 0, 1, 1], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], bool)
    assert np.array_equal(M.cityscapes_ignore(raw, CLASS_OF_LABEL), want)
    import torch
    from rsis_amd.dataloader.cityscapes import ignore_from_ids
    assert np.array_equal(ignore_from_ids(torch.from_numpy(raw)[None]).numpy()[0], want)


def test_coco_rule_on_a_hand_written_file():
    """6 x 8 image: a crowd as run counts over columns 2..5 of rows 1..4, a polygon crowd over the right edge, an instance painted at
    (2..3, 3..4): the map is their union minus the instance, then read through flipped, strided tables"""
    h, w = 6, 8
    m = np.zeros((h, w), np.uint8)
    m[1:5, 2:6] = 1
    v = m.T.reshape(-1)
    edges = np.flatnonzero(np.diff(v)) + 1
    counts = np.diff(np.concatenate([[0], edges, [len(v)]])).tolist()
    ann = dict(images=[dict(id=7, height=h, width=w)], categories=[dict(id=1, name="a")],
               annotations=[dict(image_id=7, iscrowd=1, segmentation=dict(size=[h, w], counts=counts)),
                            dict(image_id=7, iscrowd=1, segmentation=[[6.0, 0.0, 8.0, 0.0, 8.0, 6.0, 6.0, 6.0]]),
                            dict(image_id=7, iscrowd=0, segmentation=[[3.0, 2.0, 5.0, 2.0, 5.0, 4.0, 3.0, 4.0]])])
    ins = np.zeros((h, w), np.int32)
    ins[2:4, 3:5] = 1
    full = M.coco_ignore(ann, 7, np.arange(h), np.arange(w), ins)
    want = m.copy()
    want[:, 6:8] = 1
    want[2:4, 3:5] = 0
    assert np.array_equal(full, want)
    sy, sx = np.array([0, 2, 4]), np.arange(w)[::-1][::2]                 # rows 0, 2, 4; columns 7, 5, 3, 1
    assert np.array_equal(M.coco_ignore(ann, 7, sy, sx, ins[sy][:, sx]), want[sy][:, sx])


def test_torch_fallback_states_the_same_definition():
    """utils.hungarian.softIoU_matrix / softIoU with keep= (what runIter uses where the kernels refuse the shapes) against the float64
    statement; N = 19 is such a shape (not a multiple of 8)"""
    import torch
    from rsis_amd.utils.hungarian import softIoU, softIoU_matrix
    rs = np.random.default_rng(9)
    B, T, G, N = 2, 3, 4, 19
    logits = rs.normal(0, 2, (B, T, N)).astype(np.float32)
    y = (rs.random((B, G, N)) < 0.5).astype(np.float32)
    ign = (rs.random((B, N)) < 0.4).astype(np.uint8)
    y[np.broadcast_to((ign != 0)[:, None, :], y.shape)] = 1
    cost, _den = L.cost64(C.sums64_ignore(L.sigmoid64(logits), y, ign))                   # (B, G, T)
    keep = (torch.from_numpy(ign) == 0).double()
    got = softIoU_matrix(torch.from_numpy(y).double(), torch.from_numpy(logits).double(), keep=keep).numpy()
    assert np.abs(got - cost).max() < 1e-12
    perm = np.stack([rs.permutation(G)[:T] for _ in range(B)])
    yp = np.stack([y[b, perm[b]] for b in range(B)])
    rows = softIoU(torch.from_numpy(yp).double().reshape(-1, N), torch.from_numpy(logits).double().reshape(-1, N),
                   keep=keep.unsqueeze(1).expand(-1, T, -1).reshape(-1, N)).numpy().reshape(B, T)
    assert np.abs(rows - cost[np.arange(B)[:, None], perm, np.arange(T)[None, :]]).max() < 1e-12
    assert np.abs(softIoU_matrix(torch.from_numpy(y).double(), torch.from_numpy(logits).double()).numpy() - cost).max() > 1e-3


def test_evaluation_drivers_switch_the_flag_off(capsys):
    """the drivers share the parser: EvalDriver opens its readers and synthetic loader without the map (5-tuples) and says so"""
    from rsis_amd.args import get_parser
    from rsis_amd.eval_common import EvalDriver
    a = get_parser().parse_args(["--synthetic", "--ignore_regions"])
    d = EvalDriver(a)
    assert d.args.ignore_regions is False and "--ignore_regions" in capsys.readouterr().err
    EvalDriver(get_parser().parse_args(["--synthetic"]))
    assert capsys.readouterr().err == ""
