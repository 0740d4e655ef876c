"""Host side of the CVPPP evaluation (no GPU): the numpy statement of the measures (tests/cvppp_golden.py) against cases computed by
hand and against the fixture it wrote; the table writer against a literal text; the file layer of rsis_amd.cvppp_eval with the
scoring function injected; the pool / job-table builder."""
import os
import warnings

import numpy as np
import pytest

import cvppp_golden as G
from rsis_amd import cvppp_eval as E

NAN = float("nan")
# (in, gt) -> {SymmetricBestDice, FgBgDice, AbsDiffFGLabels, DiffFGLabels, BestDice(in, gt), BestDice(gt, in)}, by hand:
HAND = [
    # in {0, 1, 3}: i = 0 -> Dice(0, 0) = 2*2 / (2+2) = 1; i = 1 -> 1; i = 2 does not occur: 0, still in the divisor; i = 3 -> Dice(3, 2) =
    # 2*1 / (1+1) = 1: 3 / 4.  The other way every label of {0, 1, 2} finds its twin: 1.  Foregrounds {1, 3} and {1, 2} are the same pixels.
    ([[0, 0, 1, 3]], [[0, 0, 1, 2]], [0.75, 1.0, 1.0, 1.0, 0.75, 1.0]),
    # both constant: one label each way, Dice(5, 9) = 2*6 / (6+6) = 1; both foregrounds empty: 0 / 0
    ([[5, 5, 5], [5, 5, 5]], [[9, 9, 9], [9, 9, 9]], [1.0, NAN, 0.0, 0.0, 1.0, 1.0]),
    # all-zero result (n_0 = 4) against gt with m = (1, 2, 1): Dice(0, j) = 2/5, 4/6, 2/5 -> BestDice(in, gt) = 4/6 over a range of one value;
    # BestDice(gt, in) = (2/5 + 4/6 + 2/5) / 3 added in this order; the result has no foreground: 2*0 / (0 + 3); 0 labels against 2
    ([[0, 0], [0, 0]], [[0, 1], [1, 2]], [(2 / 5 + 4 / 6 + 2 / 5) / 3, 0.0, 2.0, -2.0, 4 / 6, (2 / 5 + 4 / 6 + 2 / 5) / 3]),
]


def test_numpy_statement_against_hand_computed_cases():
    for a, g, want in HAND:
        got = G.scores(np.array(a, np.uint8), np.array(g, np.uint8))
        assert G.same_scores(got, np.array(want)), (a, g, got, want)


def test_numpy_statement_details():
    # 0 / 0 is 0 and never wins; a value of the range that does not occur counts in the divisor on either side
    assert G.dice(0, 0, 0) == 0.0 and G.dice(3, 4, 2) == 1.0
    a, g = np.array([[0, 4]], np.uint8), np.array([[0, 1]], np.uint8)
    assert G.scores(a, g)[4] == 2.0 / 5.0 and G.scores(a, g)[5] == 1.0 and G.scores(a, g)[3] == 3.0
    # the lowest value present is the background, whatever it is
    b = np.array([[7, 7, 8, 9]], np.uint8)
    assert G.same_scores(G.scores(b, b), np.array([1.0, 1.0, 0.0, 0.0, 1.0, 1.0]))
    t = G.counts(a, g)
    assert t.sum() == 2 and t[0, 0] == 1 and t[4, 1] == 1
    # the nearest rule: 2 -> 4 doubles every pixel, 4 -> 2 takes the pixels at centres 1 and 3 (floor(0.5 * 2) = 1, floor(1.5 * 2) = 3)
    assert G.nearest_resize(np.array([[1, 2]], np.uint8), 1, 4).tolist() == [[1, 1, 2, 2]]
    assert G.nearest_resize(np.array([[1, 2, 3, 4]], np.uint8), 1, 2).tolist() == [[2, 4]]
    assert [int(v) for v in E.nearest_index(3, 7)] == [min(int(np.floor((d + 0.5) * 3 / 7)), 2) for d in range(7)]


def test_fixture_matches_the_numpy_statement():
    cases = G.load()
    names = [c["name"] for c in cases]
    assert len(cases) >= 12 and {"identical", "gap_0_1_3_vs_0_1_2", "all_zero_result", "both_constant", "background_7", "labels_0_and_255",
                                 "forty_leaves", "synthesized_shifted"} <= set(names)
    for c in cases:
        assert c["in"].dtype == np.uint8 and max(c["in"].shape[0], c["gt"].shape[0]) <= 96 and max(c["in"].shape[1], c["gt"].shape[1]) <= 112
        a = c["in"] if c["in"].shape == c["gt"].shape else G.nearest_resize(c["in"], *c["gt"].shape)
        assert np.array_equal(G.counts(a, c["gt"]), c["counts"]), c["name"]
        assert G.same_scores(G.scores(c["in"], c["gt"]), c["scores"]), c["name"]
    by = dict((c["name"], c) for c in cases)
    assert G.same_scores(by["identical"]["scores"], np.array([1.0, 1.0, 0.0, 0.0, 1.0, 1.0]))
    assert G.same_scores(by["gap_0_1_3_vs_0_1_2"]["scores"], np.array(HAND[0][2]))
    assert G.same_scores(by["both_constant"]["scores"], np.array(HAND[1][2]))
    assert G.same_scores(by["all_zero_result_tiny"]["scores"], np.array(HAND[2][2]))
    assert by["background_7"]["gt"].min() == 7 and sorted(np.unique(by["labels_0_and_255"]["gt"])) == [0, 255]
    assert by["forty_leaves"]["gt"].max() == 40 and os.path.getsize(G.PATH) < 64 * 1024


EXPECTED_TABLE = """Results for images: A1

number, SymmetricBestDice, FGBGDice, AbsDiffFGLabels, DiffFGLabels
3, 0.750000, 1.000000, 1, 1
17, 1.000000, NaN, 0, 0
161, 0.488889, 0.000000, 2, -2

mean, 0.746296, NaN, 1.000000, -0.333333
std, 0.255576, NaN, 1.000000, 1.527525
median, 0.750000, NaN, 1.000000, 0.000000
max, 1.000000, NaN, 2.000000, 1.000000
min, 0.488889, NaN, 0.000000, -2.000000
"""


def test_result_table_text_and_summary(tmp_path):
    scores = np.array([h[2] for h in HAND])
    assert E.result_table_text([3, 17, 161], scores) == EXPECTED_TABLE
    name = E.write_result_table(str(tmp_path / "out"), "someone", [3, 17, 161], scores)
    assert os.path.basename(name) == "someone_A1_results.csv" and open(name).read() == EXPECTED_TABLE
    s = E.summary(scores[[0, 2]])
    assert s.shape == (5, 4) and s[0, 0] == (0.75 + scores[2, 0]) / 2 and s[1, 2] == np.std([1.0, 2.0], ddof=1) and s[3, 3] == 1.0 and s[4, 3] == -2.0
    assert np.isnan(E.summary(scores[:1])[1]).all() and E.summary(scores[:1])[0, 0] == 0.75       # one image: no sample deviation


def _png(path, a, mode=None):
    from PIL import Image
    im = Image.fromarray(a) if mode is None else Image.fromarray(a, mode=mode)
    im.save(path)
    return str(path)


def test_file_layer_with_injected_scoring(tmp_path):
    from PIL import Image
    gt, res = tmp_path / "gt", tmp_path / "res"
    gt.mkdir()
    res.mkdir()
    rng = np.random.default_rng(0)
    labels = {k: rng.integers(0, 4, (6, 7)).astype(np.uint8) for k in (2, 10, 33)}
    for k, a in labels.items():
        _png(gt / ("plant%03d_label.png" % k), a)
        _png(gt / ("plant%03d_rgb.png" % k), np.zeros((6, 7, 3), np.uint8))              # not a label file: never read
    pal = Image.fromarray(labels[10])
    pal.putpalette([v for k in range(256) for v in (k, 255 - k, 7)])                     # a palette PNG is read as its indices
    pal.save(str(res / "plant010_label.png"))
    assert Image.open(str(res / "plant010_label.png")).mode == "P"
    _png(res / "ara2012_plant2_label.png", labels[2][::-1].copy())                       # plant number = LAST number of the name
    _png(res / "plant099_label.png", labels[2])                                          # no such ground truth: ignored
    seen = {}

    def score_fn(ins, gts):
        seen["ins"], seen["gts"] = [np.asarray(a) for a in ins], [np.asarray(g) for g in gts]
        return G.score_pairs(ins, gts)
    numbers, scores = E.evaluate_dirs(str(res), str(gt), score_fn=score_fn)
    assert numbers == [2, 10, 33] and tuple(scores.shape) == (3, 6)
    assert np.array_equal(seen["gts"][0], labels[2]) and np.array_equal(seen["ins"][0], labels[2][::-1])
    assert np.array_equal(seen["ins"][1], labels[10]) and float(scores[1, 0]) == 1.0
    assert not seen["ins"][2].any() and seen["ins"][2].shape == (6, 7)                   # missing result: an all-zero image
    assert G.same_scores(scores.numpy(), G.score_pairs(seen["ins"], seen["gts"]))
    assert E.plant_number("/x/12/plant007_label.png") == 7
    # A1 sub-folders are found as well
    (tmp_path / "sub" / "A1").mkdir(parents=True)
    _png(tmp_path / "sub" / "A1" / "plant002_label.png", labels[2])
    n2, s2 = E.evaluate_dirs(str(tmp_path / "sub"), str(gt), score_fn=score_fn)
    assert n2 == numbers and float(s2[0, 0]) == 1.0
    with pytest.raises(ValueError, match="two result files"):
        E.evaluate_files([str(res / "plant010_label.png"), str(res / "plant010_label.png")], [str(gt / "plant010_label.png")], score_fn)
    with pytest.raises(ValueError, match="no \\*_label.png"):
        E.evaluate_dirs(str(res), str(tmp_path / "sub" / "A1" / "nothing"), score_fn=score_fn)


def test_refused_formats(tmp_path):
    g = _png(tmp_path / "plant001_label.png", np.zeros((4, 4), np.uint8))
    rgb = _png(tmp_path / "plant001_colour_label.png", np.zeros((4, 4, 3), np.uint8))
    deep = _png(tmp_path / "plant001_deep_label.png", np.zeros((4, 4), np.uint16))
    for bad in (rgb, deep):
        with pytest.raises(ValueError, match="8-bit greyscale .* or palette .* only"):
            E.read_label_png(bad)
        with pytest.raises(ValueError, match="refused"):
            E.evaluate_files([bad], [g], G.score_pairs)
    assert E.read_label_png(g).shape == (4, 4)


def test_job_table_and_pool_layout():
    blocks_of = lambda n: (n + 32767) // 32768
    npix = [1, 15, 17, 1961, 500 * 530, 40000]
    jobs, length, blocks = E.job_table(npix, align=16, blocks_of=blocks_of)
    assert jobs.shape == (6, 8) and jobs.dtype == np.int64 and not jobs[:, 5:].any()
    end = 0
    for p, n in enumerate(npix):
        i, g, m, t, b = (int(v) for v in jobs[p, :5])
        assert m == n and i % 16 == 0 and g % 16 == 0 and i >= end and g >= i + n and t == p * 65536
        assert b == sum(blocks_of(k) for k in npix[:p])
        end = g + n
    assert length == end and blocks == sum(blocks_of(k) for k in npix) == 1 + 1 + 1 + 1 + 9 + 2
    # align = 1: back to back, pairs start anywhere
    jobs1, length1, blocks1 = E.job_table(npix, align=1, blocks_of=blocks_of)
    assert length1 == 2 * sum(npix) and blocks1 == blocks
    assert [int(v) for v in jobs1[:, 0]] == [2 * sum(npix[:p]) for p in range(6)]
    assert [int(v) for v in jobs1[:, 1]] == [2 * sum(npix[:p]) + npix[p] for p in range(6)]
    assert any(int(v) % 16 for v in jobs1[:, 0]) and any((int(a) - int(b)) % 16 for a, b in zip(jobs1[:, 0], jobs1[:, 1]))
    for bad in ([0], [1 << 32]):
        with pytest.raises(ValueError):
            E.job_table(bad, blocks_of=blocks_of)
    # the library's own block count (callable without a GPU) is what the builder uses by default
    from rsis_amd import _lib
    L = _lib.lib()
    assert L.rsis_label_contingency_blocks(1) == 1 and L.rsis_label_contingency_blocks(0) == 0 and L.rsis_label_contingency_blocks(1 << 32) == 0
    n = L.rsis_label_contingency_blocks(2448 * 2048)
    assert n >= 64 and E.job_table([2448 * 2048, 7])[0][1, 4] == n
    # arguments are checked before anything is launched (no device is touched here)
    assert L.rsis_label_contingency_batch(None, 16, None, 1, 1, None, 65536, None) == 1
    assert L.rsis_label_scores_batch(None, 65536, None, 1, None, None) == 1


def test_entry_points_need_the_gpu():
    import torch
    a = [torch.zeros((2, 2), dtype=torch.uint8)]
    if not torch.cuda.is_available():                              # (with a device the same calls are tests/test_gpu_cvppp.py's)
        with pytest.raises(RuntimeError, match="needs the GPU"):
            E.score_pairs(a, a)
        with pytest.raises(SystemExit, match="needs the GPU"):
            E.main(["--results", "x", "--gt", "y"])
    with pytest.raises(ValueError, match="2-d uint8"):
        E._as_label_tensor(torch.zeros((2, 2)), "in[0]")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert E.resize_nearest(torch.tensor([[1, 2]], dtype=torch.uint8), 1, 4).tolist() == [[1, 1, 2, 2]]
