"""Host half of reading standard COCO ground truth (rsis_amd/cocoeval.py: segmentation_kind, load_coco_file) and the polygon fixture
tests/golden/polymask.npz (tools/make_golden_polymask.py, from the reference's own C mask API): no GPU needed.  The fixture is
checked for internal consistency, and a float64 numpy statement of the toggle-parity rule (tests/polymask_golden.py) must reproduce
every part of it -- the rule rsis_amd/csrc/polymask.hip runs on the device."""
import json

import numpy as np
import pytest

import polymask_golden as PG
from rsis_amd import cocoeval as CE


def test_segmentation_kind_accepts_the_three_forms():
    assert CE.segmentation_kind({"size": [4, 5], "counts": "04"}) == "rle"
    assert CE.segmentation_kind({"size": [4, 5], "counts": b"04"}) == "rle"
    assert CE.segmentation_kind({"size": [4, 5], "counts": [3, 2, 15]}) == "counts"
    assert CE.segmentation_kind({"size": (4, 5), "counts": (20,)}) == "counts"
    assert CE.segmentation_kind([[1, 2, 3.5, 4, 5, 6]]) == "polygons"
    assert CE.segmentation_kind([[1, 2, 3, 4, 5, 6], [0.5, 0.5, 9, 1, 4, 7.25, 2, 2]]) == "polygons"
    assert CE.segmentation_kind([[-100.0, 2, 3, 4e6, 5, 6]]) == "polygons"         # outside the image is legal
    assert CE.segmentation_kind([[1, 2, 3, 4, 5, (2.0 ** 30 - 3) / 5]]) == "polygons"


@pytest.mark.parametrize("seg", [
    [10, 20, 30, 40],                                               # a bare box
    [1, 2, 3, 4, 5, 6],                                             # a bare list of numbers: parts must be lists
    [],                                                             # no part
    [[]],
    [[1, 2, 3, 4]],                                                 # two points
    [[1, 2, 3, 4, 5, 6, 7]],                                        # an odd count
    [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4]],                             # the second part is short
    [[1, 2, 3, 4, 5, float("nan")]],
    [[1, 2, 3, 4, float("inf"), 6]],
    [[1, 2, 3, 4, 5, 2.0 ** 30 / 5]],                               # |5 * coordinate| reaches 2^30
    [[1, 2, 3, 4, 5, -(2.0 ** 30) / 5]],
    [[1, 2, 3, 4, 5, "x"]],
    [[1, 2, 3, 4, 5, None]],
    {"counts": "04"},                                               # no size
    {"size": [4, 5]},                                               # no counts
    {"size": [4, 5], "counts": 7},
    None,
    "04",
    7,
])
def test_segmentation_kind_refuses(seg):
    with pytest.raises(ValueError):
        CE.segmentation_kind(seg)


def test_load_coco_file(tmp_path):
    recs = [{"image_id": 1, "category_id": 2, "segmentation": [[1, 2, 3, 4, 5, 6]]}]
    images = [{"id": 1, "height": 10, "width": 12}]
    p = tmp_path / "list.json"
    p.write_text(json.dumps(recs))
    assert CE.load_coco_file(str(p)) == (recs, None)
    p = tmp_path / "dict.json"
    p.write_text(json.dumps({"annotations": recs, "images": images, "categories": []}))
    assert CE.load_coco_file(str(p)) == (recs, images)
    p = tmp_path / "noimages.json"
    p.write_text(json.dumps({"annotations": recs}))
    assert CE.load_coco_file(str(p)) == (recs, None)
    a = CE.get_cli_parser().parse_args(["--gt", "g.json", "--dt", "p.json", "--all_images"])
    assert a.all_images and not CE.get_cli_parser().parse_args(["--gt", "g.json", "--dt", "p.json"]).all_images


def test_fixture_is_consistent():
    F = PG.load()
    names = [r["name"] for r in F["records"]]
    for want in ("size_13x11", "size_300x7", "one_word_column", "h_is_1", "w_is_1", "outside_every_side", "clamped_to_h_mid_column",
                 "position_hw_dropped", "entirely_outside", "repeated_consecutive_vertex", "repeated_first_last_vertex",
                 "three_collinear_points", "half_integer_coordinates", "integer_coordinates", "bow_tie", "three_parts_two_overlap",
                 "circle_1500_vertices", "long_edge_star"):
        assert want in names
    for r in F["records"]:
        n = r["h"] * r["w"]
        assert CE.segmentation_kind([p.tolist() for p in r["parts"]]) == "polygons"
        parts = [PG.decode(c, n) for c in r["part_counts"]]         # (decode asserts that the counts sum to h * w)
        assert [int(m.sum()) for m in parts] == r["part_area"], r["name"]
        merged = PG.decode(r["counts"], n)
        union = np.zeros((n,), np.uint8)
        for m in parts:
            union |= m
        assert np.array_equal(merged, union) and int(merged.sum()) == r["area"], r["name"]
    r = F["records"][names.index("three_parts_two_overlap")]
    parts = [PG.decode(c, r["h"] * r["w"]) for c in r["part_counts"]]
    assert not np.array_equal(parts[0] ^ parts[1] ^ parts[2], PG.decode(r["counts"], r["h"] * r["w"]))
    assert F["records"][names.index("entirely_outside")]["area"] == 0
    for u in F["urle"]:
        m = PG.decode(u["counts"], u["h"] * u["w"])
        assert int(m.sum()) == u["area"], u["name"]
        assert np.array_equal(CE.rle_from_string(u["string"]), u["counts"]), u["name"]
    un = {u["name"]: u for u in F["urle"]}
    assert un["leading_zero_count"]["counts"][0] == 0 and un["all_zero"]["area"] == 0
    assert len(un["odd_number_of_counts"]["counts"]) % 2 == 1 and len(un["even_number_of_counts"]["counts"]) % 2 == 0
    ev = F["eval"]
    assert len(ev["gt_poly"]) == len(ev["gt_rle"]) and len(ev["images"]) == 6
    kinds = [CE.segmentation_kind(r["segmentation"]) for r in ev["gt_poly"]]
    assert kinds.count("counts") == 1 and kinds.count("polygons") == len(kinds) - 1
    assert all(CE.segmentation_kind(r["segmentation"]) == "rle" for r in ev["gt_rle"] + ev["dt"])


def test_toggle_parity_rule_reproduces_every_fixture_part():
    F = PG.load()
    nparts = 0
    for r in F["records"]:
        h, w = r["h"], r["w"]
        for p, c in zip(r["parts"], r["part_counts"]):
            assert np.array_equal(PG.part_mask(p, h, w), PG.decode(c, h * w)), r["name"]
            nparts += 1
        assert np.array_equal(PG.record_mask(r["parts"], h, w), PG.decode(r["counts"], h * w)), r["name"]
    assert nparts >= 40
