"""Host half of the COCO segm evaluation (rsis_amd/cocoeval.py) against the reference's own COCOeval (tests/golden/cocoeval.npz):
no GPU needed -- the RLE text functions of the library are host code, accumulate / summarize are numpy."""
import io
import os

import numpy as np

from cocoeval_golden import load, per_k_from_cells
from rsis_amd import cocoeval as CE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_rle_text_round_trip():
    z = np.load(os.path.join(GOLDEN, "rle.npz"))
    for k in range(int(z["n"])):
        counts, text = z["counts%d" % k], bytes(z["string%d" % k])
        got = CE.rle_from_string(text)
        assert got.dtype == np.uint32 and np.array_equal(got, counts), k
        assert CE.rle_to_string(counts) == text, k
        assert np.array_equal(CE.rle_from_string(text.decode("ascii")), counts)
    sets, _ = load()
    for r in sets[0]["gt"] + sets[0]["dt"]:                        # and on strings of the reference's encoder
        c = CE.rle_from_string(r["segmentation"]["counts"])
        assert int(c.sum()) == r["segmentation"]["size"][0] * r["segmentation"]["size"][1]
        assert int(c[1::2].sum()) == int(r["area"])
        assert CE.rle_to_string(c).decode("ascii") == r["segmentation"]["counts"]


def _params(run):
    p = CE.Params()
    p.maxDets = sorted(run["maxDets"])
    p.useCats = run["useCats"]
    return p


def test_accumulate_and_summarize_reproduce_the_reference():
    _, runs = load()
    assert len(runs) >= 5
    for run in runs:
        p = _params(run)
        assert len(p.iouThrs) == 10 and len(p.recThrs) == 101
        precision, recall = CE.accumulate_cells(per_k_from_cells(run), p.maxDets, p.recThrs, 10, 4)
        assert precision.shape == run["precision"].shape and precision.dtype == np.float64
        assert np.array_equal(precision, run["precision"])
        assert np.array_equal(recall, run["recall"])
        text = io.StringIO()
        stats = CE.summarize_stats(precision, recall, p, text)
        assert stats.shape == (13,)
        assert np.abs(stats - run["stats"]).max() <= 1e-11
        lines = text.getvalue().splitlines()
        assert len(lines) == 13 and lines == run["summary"]


def test_duplicate_max_dets_column_is_kept():
    """maxDets = [1, 100, 100]: accumulate keeps both columns, summarize selects by equality (averages two identical columns)"""
    _, runs = load()
    run = [r for r in runs if r["maxDets"] == [1, 100, 100]][0]
    precision, _ = CE.accumulate_cells(per_k_from_cells(run), [1, 100, 100], CE.Params().recThrs, 10, 4)
    assert precision.shape[-1] == 3 and np.array_equal(precision[..., 1], precision[..., 2])


def test_category_without_ground_truth_is_minus_one():
    _, runs = load()
    assert (runs[0]["precision"][:, :, 4] == -1).all()
    precision, recall = CE.accumulate_cells(per_k_from_cells(runs[0]), [1, 10, 100], CE.Params().recThrs, 10, 4)
    assert (precision[:, :, 4] == -1).all() and (recall[:, 4] == -1).all()


def test_cli_parses():
    a = CE.get_cli_parser().parse_args(["--gt", "g.json", "--dt", "p.json", "-max_dets", "10", "--ignore_cats", "--all_classes"])
    assert (a.gt, a.dt, a.max_dets, a.use_cats, a.all_classes) == ("g.json", "p.json", 10, False, True)
    b = CE.get_cli_parser().parse_args(["--gt", "g.json", "--dt", "p.json"])
    assert b.max_dets == 100 and b.use_cats and not b.all_classes
    assert CE.words_of(1) == 2 and CE.words_of(128) == 2 and CE.words_of(129) == 4
