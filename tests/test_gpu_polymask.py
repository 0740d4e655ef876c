"""Polygon and uncompressed-RLE ground truth on the device (rsis_amd/csrc/polymask.hip, rsis_amd/cocoeval.py) against the reference's
own C mask API (tests/golden/polymask.npz, tools/make_golden_polymask.py): masks are compared BIT FOR BIT with the decoded run counts
of rleFrPoly / rleMerge, areas with rleArea, and an evaluation whose ground truth comes as polygons / counts must give exactly the
numbers it gives from the same masks as compressed RLE.  There is no tolerance anywhere."""
import io
import json

import numpy as np
import pytest
import torch

import polymask_golden as PG
from rsis_amd import cocoeval as CE

pytestmark = pytest.mark.gpu


def _unpack(row, length):
    w = row.cpu().numpy().view(np.uint64)
    b = np.unpackbits(w.view(np.uint8), bitorder="little")
    assert not b[length:].any(), "tail bits must be zero"
    return b[:length]


@pytest.fixture(scope="module")
def fixture():
    return PG.load()


@pytest.fixture(scope="module")
def batched(fixture):
    """every fixture record, then every part as a record of its own, in ONE call"""
    recs = fixture["records"]
    polys = [[p for p in r["parts"]] for r in recs] + [[p] for r in recs for p in r["parts"]]
    sizes = [(r["h"], r["w"]) for r in recs] + [(r["h"], r["w"]) for r in recs for _p in r["parts"]]
    rows, area = CE.poly_to_bits(polys, sizes)
    torch.cuda.synchronize()
    return rows, area.cpu().tolist()


def test_masks_equal_the_reference_bit_for_bit(fixture, batched):
    rows, area = batched
    recs = fixture["records"]
    assert len(rows) == len(area) == len(recs) + sum(len(r["parts"]) for r in recs)
    k = len(recs)
    for j, r in enumerate(recs):
        n = r["h"] * r["w"]
        assert rows[j].dtype == torch.int64 and rows[j].shape == (CE.words_of(n),)
        assert np.array_equal(_unpack(rows[j], n), PG.decode(r["counts"], n)), r["name"]
        assert area[j] == r["area"], r["name"]
        for c, a in zip(r["part_counts"], r["part_area"]):
            assert np.array_equal(_unpack(rows[k], n), PG.decode(c, n)), r["name"]
            assert area[k] == a, r["name"]
            k += 1


def test_one_call_each_equals_the_batched_call(fixture, batched):
    """grouped offsets, and the scratch row is zeroed per record and per part"""
    rows, area = batched
    for j, r in enumerate(fixture["records"]):
        one, a = CE.poly_to_bits([r["parts"]], [(r["h"], r["w"])])
        assert len(one) == 1 and torch.equal(one[0], rows[j]) and a.cpu().tolist() == [area[j]], r["name"]
    rows2, area2 = CE.poly_to_bits([r["parts"] for r in reversed(fixture["records"])], [(r["h"], r["w"]) for r in reversed(fixture["records"])])
    n = len(fixture["records"])
    assert all(torch.equal(rows2[n - 1 - j], rows[j]) for j in range(n)) and area2.cpu().tolist() == area[:n][::-1]
    assert CE.poly_to_bits([], [])[0] == []


def test_uncompressed_counts_equal_their_compressed_form(fixture):
    """_add_records hands a list of counts straight to rle_to_bits: the same row as from the reference's text of the same mask"""
    for u in fixture["urle"]:
        size = [u["h"], u["w"]]
        ev = CE.COCOEvalDevice()
        ev.add_gt([{"image_id": 1, "category_id": 1, "segmentation": {"size": size, "counts": [int(v) for v in u["counts"]]}},
                   {"image_id": 1, "category_id": 1, "segmentation": {"size": size, "counts": u["string"]}}])
        (bits, area), = ev._gt.chunks[1]
        assert bits.shape[0] == 2 and torch.equal(bits[0], bits[1]) and area.cpu().tolist() == [u["area"]] * 2, u["name"]
        assert np.array_equal(_unpack(bits[0], u["h"] * u["w"]), PG.decode(u["counts"], u["h"] * u["w"])), u["name"]
    with pytest.raises(ValueError):                                 # counts that do not sum to h * w
        CE.COCOEvalDevice().add_gt([{"image_id": 1, "category_id": 1, "segmentation": {"size": [4, 5], "counts": [3, 2, 14]}}])


def _score(gt, dt, images, cats):
    ev = CE.COCOEvalDevice(gt, dt, images=images)
    ev.params.catIds = list(cats)
    ev.evaluate().accumulate().summarize(io.StringIO())
    return ev


def test_evaluation_from_polygons_equals_evaluation_from_rle(fixture, tmp_path):
    E = fixture["eval"]
    a = _score(E["gt_poly"], E["dt"], E["images"], E["cats"])
    b = _score(E["gt_rle"], E["dt"], None, E["cats"])
    assert a.params.imgIds == b.params.imgIds and len(a.params.imgIds) == 6
    assert np.array_equal(a.stats, b.stats) and (np.asarray(a.stats)[[0, 1, 7]] > 0).all()
    assert np.array_equal(a.eval["precision"], b.eval["precision"]) and np.array_equal(a.eval["recall"], b.eval["recall"])
    # sizes as {image id: (h, w)}, and given to add_gt
    c = CE.COCOEvalDevice()
    c.add_gt(E["gt_poly"], images={im["id"]: (im["height"], im["width"]) for im in E["images"]})
    c.add_dt(E["dt"])
    c.params.imgIds, c.params.catIds = list(b.params.imgIds), list(E["cats"])
    c.evaluate().accumulate().summarize(io.StringIO())
    assert np.array_equal(c.stats, b.stats) and np.array_equal(c.eval["precision"], b.eval["precision"])
    # the same through the command line, on two JSON files per form
    paths = {}
    for name, obj in (("gt_poly", {"images": E["images"], "annotations": E["gt_poly"]}), ("gt_rle", E["gt_rle"]), ("dt", E["dt"])):
        paths[name] = str(tmp_path / (name + ".json"))
        with open(paths[name], "w") as f:
            json.dump(obj, f)
    ra = CE.main(["--gt", paths["gt_poly"], "--dt", paths["dt"], "--all_classes"])
    rb = CE.main(["--gt", paths["gt_rle"], "--dt", paths["dt"], "--all_classes"])
    # (main runs the reference's protocol, maxDets = [1, 100, 100]: its numbers are compared with each other, not with those above)
    assert ra == rb and len(ra["stats"]) == 13 and ra["stats"][0] > 0 and sorted(ra["per_class"]) == ["1", "2", "3"]
    # --all_images: the images come from the file; here every image has ground truth, so the numbers stay
    rc = CE.main(["--gt", paths["gt_poly"], "--dt", paths["dt"], "--all_images"])
    assert rc["stats"] == rb["stats"]
    # ... and with the ground truth of one image taken away, its detections count (as false positives) only under --all_images
    last = E["images"][-1]["id"]
    fewer = [r for r in E["gt_poly"] if r["image_id"] != last]
    assert len(fewer) < len(E["gt_poly"]) and any(r["image_id"] == last for r in E["dt"])
    with open(paths["gt_poly"], "w") as f:
        json.dump({"images": E["images"], "annotations": fewer}, f)
    rd = CE.main(["--gt", paths["gt_poly"], "--dt", paths["dt"]])
    re_ = CE.main(["--gt", paths["gt_poly"], "--dt", paths["dt"], "--all_images"])
    want = {}
    for key, ids in (("gt", sorted(set(r["image_id"] for r in fewer))), ("all", sorted(im["id"] for im in E["images"]))):
        ev = CE.COCOEvalDevice([r for r in E["gt_rle"] if r["image_id"] != last], E["dt"])
        want[key] = CE.run_reference_protocol(ev, ids, E["cats"], 100, True, False, out=io.StringIO())
    print("AP without / with --all_images: %.17g %.17g" % (rd["stats"][0], re_["stats"][0]))
    assert rd == want["gt"] and re_ == want["all"]


def test_polygon_sizes_known_missing_and_conflicting(fixture):
    E = fixture["eval"]
    poly = [r for r in E["gt_poly"] if isinstance(r["segmentation"], list)][0]
    img = poly["image_id"]
    h, w = [(im["height"], im["width"]) for im in E["images"] if im["id"] == img][0]
    with pytest.raises(ValueError, match=repr(img)):
        CE.COCOEvalDevice([poly], None)                             # no size known for the image
    with pytest.raises(ValueError, match=repr(img)):
        CE.COCOEvalDevice([poly], None, images={img + 1: (h, w)})
    # a size known from an RLE record of the image, on the other side
    dt = [r for r in E["dt"] if r["image_id"] == img]
    ev = CE.COCOEvalDevice()
    ev.add_dt(dt)
    ev.add_gt([poly])
    want = CE.COCOEvalDevice([r for r in E["gt_rle"] if r["id"] == poly["id"]])
    assert torch.equal(ev._gt.chunks[img][0][0], want._gt.chunks[img][0][0])
    # conflicts: `images` against an RLE record, and against a size given before
    with pytest.raises(ValueError, match="different sizes"):
        CE.COCOEvalDevice([poly], dt, images={img: (h + 1, w)})
    with pytest.raises(ValueError, match="different sizes"):
        ev.add_gt([poly], images=[{"id": img, "height": w + 3, "width": h}])
    with pytest.raises(ValueError):                                 # a refused segmentation is refused on the host, before any launch
        CE.COCOEvalDevice([dict(poly, segmentation=[[1.0, 2.0, 3.0, 4.0]])], None, images={img: (h, w)})
