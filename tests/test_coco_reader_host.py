"""CPU tests of the COCO reader (rsis_amd/dataloader/coco.py): the parsing rules, the index tables against scipy's zoom, the synthesized
tree, the flags, and the new symbol in header, library and binding.  Every comparison is exact."""
import argparse
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_reader_cases as C  # noqa: E402
import polymask_golden as PG  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(d, **kw):
    a = argparse.Namespace(gt_maxseqlen=20, batch_size=3, coco_dir=d, coco_train_set="train2017", coco_val_set="val2017", num_classes=4,
                           rotation=10, translation=0.1, shear=0.1, zoom=0.7, crop=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from rsis_amd.dataloader.coco import synthesize_coco_dir
    return synthesize_coco_dir(str(tmp_path_factory.mktemp("coco") / "COCO"), n=4, sizes=((48, 64), (75, 50), (33, 47)), seed=3)


def _annotation(tree, name="train2017"):
    with open(os.path.join(tree, "annotations", "instances_%s.json" % name)) as f:
        return json.load(f)


def _write(tmp_path, images, anns, cats, name="train2017"):
    from PIL import Image
    d = str(tmp_path / "D")
    os.makedirs(os.path.join(d, "annotations"), exist_ok=True)
    os.makedirs(os.path.join(d, name), exist_ok=True)
    for im in images:
        Image.fromarray(np.zeros((im["height"], im["width"], 3), np.uint8)).save(os.path.join(d, name, im["file_name"]))
    with open(os.path.join(d, "annotations", "instances_%s.json" % name), "w") as f:
        json.dump({"images": images, "annotations": anns, "categories": cats}, f)
    return d


SQUARE = [2.0, 2.0, 10.0, 2.0, 10.0, 10.0, 2.0, 10.0]


def test_categories_map_by_rank_and_num_classes_is_checked(tree):
    from rsis_amd.dataloader.coco import COCO
    ds = COCO(_args(tree), split="train")
    assert ds.get_classes() == ["<eos>", "car", "cat", "bottle"] and ds.category_ids == [0, 3, 17, 44] and ds.num_classes == 4
    ann = _annotation(tree)
    for i, img_id in enumerate(ds.image_ids):
        want, _hw = C.file_sample(ann, img_id)
        got = ds.records(i)
        assert [c for _p, _i, c in got] == [c for _p, c in want] and [k for _p, k, _c in got] == list(range(1, len(want) + 1))
        for (gp, _i, _c), (wp, _c2) in zip(got, want):
            assert len(gp) == len(wp) and all(np.array_equal(a, np.asarray(b, np.float64)) for a, b in zip(gp, wp))
    with pytest.raises(ValueError, match="-num_classes must be 4"):
        COCO(_args(tree, num_classes=21), split="train")
    with pytest.raises(ValueError, match="train and val"):
        COCO(_args(tree), split="test")
    assert COCO(_args(tree), split="val").ann_file.endswith("instances_val2017.json")


def test_crowd_box_only_empty_and_crowd_only_images(tmp_path, capsys):
    from rsis_amd.dataloader.coco import COCO
    cats = [{"id": 9, "name": "b"}, {"id": 2, "name": "a"}]
    images = [{"id": 11 + k, "file_name": "%d.jpg" % k, "height": 16, "width": 20} for k in range(4)]
    crowd = {"size": [16, 20], "counts": [40, 30, 250]}
    anns = [{"id": 1, "image_id": 11, "category_id": 9, "segmentation": SQUARE, "area": 64.0, "iscrowd": 0},           # a bare list: no mask
            {"id": 2, "image_id": 11, "category_id": 9, "segmentation": [SQUARE], "area": 64.0, "iscrowd": 0},
            {"id": 3, "image_id": 11, "category_id": 2, "segmentation": crowd, "area": 30.0, "iscrowd": 1},
            {"id": 4, "image_id": 11, "category_id": 2, "segmentation": crowd, "area": 30.0, "iscrowd": 0},              # RLE, not crowd
            {"id": 5, "image_id": 11, "category_id": 2, "segmentation": [[1.0, 1.0, 5.0, 1.0]], "area": 0.0, "iscrowd": 0},
            {"id": 6, "image_id": 12, "category_id": 2, "segmentation": crowd, "area": 30.0, "iscrowd": 1},              # crowd only
            {"id": 7, "image_id": 14, "category_id": 2, "segmentation": [SQUARE, SQUARE[:6]], "area": 70.0, "iscrowd": 0}]
    d = _write(tmp_path, images, anns, cats)
    ds = COCO(_args(d, num_classes=3), split="train")
    out = capsys.readouterr()
    assert ds.get_classes() == ["<eos>", "a", "b"]
    assert ds.image_ids == [11, 14] and len(ds) == 2 and [os.path.basename(f) for f in ds.get_sample_list()] == ["0.jpg", "3.jpg"]
    assert out.err.count("warning") == 1 and "3 records" in out.err           # the bare list, the non-crowd RLE, the two-point part
    assert "2 of 4 images" in out.out
    (parts, iid, cls), = ds.records(0)
    assert iid == 1 and cls == 2 and len(parts) == 1 and np.array_equal(parts[0], np.asarray(SQUARE))
    (parts, iid, cls), = ds.records(1)
    assert iid == 1 and cls == 1 and [len(p) for p in parts] == [8, 6]
    assert ds.raw_size(0) == (16, 20) and ds.image_path(1).endswith(os.path.join("train2017", "3.jpg"))
    # get_raw_sample: the crowd pixels stay background
    _img, ins, seg = ds.get_raw_sample(0)
    want = PG.record_mask([np.asarray(SQUARE)], 16, 20).reshape(20, 16).T
    assert np.array_equal(ins, want.astype(np.int32)) and np.array_equal(seg, 2 * want.astype(np.int32)) and want.sum() > 0


def test_cap_keeps_the_255_largest_by_area_in_file_order(tmp_path):
    from rsis_amd.dataloader.coco import COCO
    cats = [{"id": 1, "name": "a"}]
    images = [{"id": 5, "file_name": "a.jpg", "height": 40, "width": 40}]
    r = np.random.default_rng(0)
    areas = r.permutation(np.repeat(np.arange(1, 151), 2)).astype(np.float64)       # 300 records, every area twice
    anns = []
    for k, a in enumerate(areas):
        x, y = float(k % 20) * 2, float(k // 20) * 2
        anns.append({"id": k + 1, "image_id": 5, "category_id": 1, "segmentation": [[x, y, x + 1.5, y, x + 1.5, y + 1.5 + 1e-3 * k]],
                     "area": float(a), "iscrowd": 0})
    ds = COCO(_args(_write(tmp_path, images, anns, cats), num_classes=2), split="train")
    got = ds.records(0)
    assert len(got) == 255 and [i for _p, i, _c in got] == list(range(1, 256))
    # 45 records leave: both of the areas 1..22 and, of the two of area 23, the LATER one in the file
    later23 = max(k for k, a in enumerate(areas) if a == 23)
    keep = [k for k, a in enumerate(areas) if a > 23 or (a == 23 and k != later23)]
    assert len(keep) == 255
    assert [float(p[0][5]) for p, _i, _c in got] == [anns[k]["segmentation"][0][5] for k in keep]


PAIRS = [(48, 16), (64, 16), (75, 32), (33, 13), (47, 17), (48, 96), (33, 80), (5, 64), (2, 7), (1, 5), (7, 1), (1, 1), (640, 256),
         (480, 256), (257, 100), (100, 257), (50, 50)]


def test_index_tables_equal_scipy_zoom_of_a_ramp():
    from rsis_amd.dataloader.coco import index_tables, zoom_index
    for n, m in PAIRS:
        sy, sx = C.ramp_tables((n, 3 + n % 4), (m, 2 + m % 5))
        assert np.array_equal(zoom_index(n, m), sy), (n, m)
        assert np.array_equal(zoom_index(3 + n % 4, 2 + m % 5), sx), (n, m)
        assert zoom_index(n, m).dtype == np.int32
    assert zoom_index(9, 1).tolist() == [0]
    native, resized = (48, 75), (32, 50)
    wy, wx = C.ramp_tables(native, resized)
    sy, sx = index_tables(native, resized)
    assert np.array_equal(sy, wy) and np.array_equal(sx, wx) and len(set(sx.tolist())) == 50
    sy, sx = index_tables(native, resized, flip=True)
    assert np.array_equal(sy, wy) and np.array_equal(sx, wx[::-1])
    sy, sx = index_tables(native, resized, flip=True, crop=(0, 7), size=(32, 32))
    assert np.array_equal(sy, wy) and np.array_equal(sx, wx[::-1][7:39])
    sy, sx = index_tables((75, 50), (48, 32), crop=(5, 0), size=(32, 32))
    wy, wx = C.ramp_tables((75, 50), (48, 32))
    assert np.array_equal(sy, wy[5:37]) and np.array_equal(sx, wx) and sy.flags["C_CONTIGUOUS"]


def test_synthesized_tree_is_what_it_claims(tree):
    from PIL import Image
    from rsis_amd.cocoeval import segmentation_kind
    from rsis_amd.dataloader.coco import COCO, compose_maps, polygon_mask
    for split, name in (("train", "train2017"), ("val", "val2017")):
        ann = _annotation(tree, name)
        ds = COCO(_args(tree), split=split)
        assert [c["id"] for c in ann["categories"]] == [3, 17, 44] and len(ann["images"]) == 6 and len(ds) == 4
        assert ds.image_ids == [im["id"] for im in ann["images"][:4]]
        assert {(im["height"], im["width"]) for im in ann["images"]} == {(48, 64), (75, 50), (33, 47)}
        by_img = {im["id"]: [a for a in ann["annotations"] if a["image_id"] == im["id"]] for im in ann["images"]}
        assert [a["iscrowd"] for a in by_img[ann["images"][4]["id"]]] == [1] and by_img[ann["images"][5]["id"]] == []
        assert sum(a["iscrowd"] for a in by_img[ann["images"][0]["id"]]) == 1
        assert all(segmentation_kind(a["segmentation"]) == ("counts" if a["iscrowd"] else "polygons") for a in ann["annotations"])
        for i, img_id in enumerate(ds.image_ids):
            with Image.open(ds.image_path(i)) as im:
                assert im.format == "JPEG" and im.size == ds.raw_size(i)[::-1]
            recs, (h, w) = C.file_sample(ann, img_id)
            masks = [PG.record_mask([np.asarray(p, np.float64) for p in parts], h, w) for parts, _c in recs]
            areas = [int(m.sum()) for m in masks]
            assert len(recs) == 6 and any(len(p) == 2 for p, _c in recs) and areas[4] == areas[5] > 0 and min(areas) > 0
            m2 = [m.reshape(w, h).T > 0 for m in masks]
            assert (m2[4] & m2[5]).any()                                        # the equal pair overlaps: the tie rule decides pixels
            assert (m2[1] & m2[0]).sum() == areas[1] and (m2[2] & m2[0]).any() and not (m2[2] & m2[0]).all()     # nested; overlapping
            assert any(abs(v - round(v)) > 0 for p, _c in recs for part in p for v in part)
            # the package's numpy rasteriser and composer equal the tests' statements; get_raw_sample is made of them
            assert all(np.array_equal(polygon_mask(parts, h, w).T.reshape(-1), m) for (parts, _c), m in zip(recs, masks))
            want = C.compose(masks, [(h, w)] * 6, range(1, 7), [c for _p, c in recs], (h, w))
            _img, ins, seg = ds.get_raw_sample(i)
            assert np.array_equal(ins, want[0]) and np.array_equal(seg, want[1]) and set(np.unique(ins).tolist()) == set(range(7))
            got = compose_maps([m.reshape(w, h).T for m in masks], range(1, 7), [c for _p, c in recs], h, w)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_host_item_and_staged_tables(tree):
    from PIL import Image
    from rsis_amd.dataloader.coco import COCO
    ann = _annotation(tree)
    ds = COCO(_args(tree), split="train", imsize=32, augment=True)
    assert ds.crop is True and ds.flip is True and ds.augmentation_transform.zoom_range == (0.7, 1.4)
    seen, items = set(), []
    for seed in range(8):
        for i in range(len(ds)):
            im, rec = ds.host_item(i, random.Random(seed))
            rng = random.Random(seed)                                          # the draws, in Pascal's order
            h, w = ds.raw_size(i)
            rh, rw = (32, max(32, int(32 * w / h))) if w > h else (max(32, int(32 * h / w)), 32)
            flip = rng.random() < 0.5
            ow = 0 if (rw - 32) // 2 <= 0 else rng.randrange((rw - 32) // 2)
            oh = 0 if (rh - 32) // 2 <= 0 else rng.randrange((rh - 32) // 2)
            assert rec == (i, (rh, rw), flip, (oh, ow)) and i in ds._cache
            with Image.open(ds.image_path(i)) as f:
                full = np.asarray(f.convert("RGB").resize((rw, rh), Image.BILINEAR)).transpose(2, 0, 1)
            full = full[:, :, ::-1] if flip else full
            assert im.dtype == np.uint8 and np.array_equal(im, full[:, oh:oh + 32, ow:ow + 32])
            seen.add((flip, oh > 0 or ow > 0))
            if seed == 3:
                items.append(rec)
    assert {True, False} == {f for f, _c in seen} and any(c for _f, c in seen)
    table, lay = ds.stage_tables(items[:3], (32, 32))
    o = lay["off"]
    assert table.dtype == np.int64 and lay["B"] == 3 and lay["n"] == 18 and lay["max_recs"] == 6 and o[-1] == len(table)
    xy, ptab, poly, paint, imgs = table[o[0]:o[1]].view(np.float64), table[o[1]:o[2]].reshape(-1, 2), table[o[2]:o[3]].reshape(-1, 8), \
        table[o[3]:o[4]].reshape(-1, 8), table[o[4]:o[5]].reshape(-1, 2)
    src = table[o[5]:o[6]].view(np.int32)
    assert imgs.tolist() == [[0, 6], [6, 6], [12, 6]] and lay["nverts"] == len(xy) // 2 == int(ptab[:, 1].sum()) and lay["nparts"] == len(ptab)
    k = 0
    for b, rec in enumerate(items[:3]):
        recs, (h, w) = C.file_sample(ann, ds.image_ids[rec[0]])
        for j, (parts, cls) in enumerate(recs):
            p0, np_, ph, pw, fw, words = poly[k][:6].tolist()
            assert (np_, ph, pw, words) == (len(parts), h, w, C.words_of(h * w)) and paint[k].tolist() == [fw, words, h, w, j + 1, cls, 0, 0]
            for q, part in enumerate(parts):
                v0, nv = ptab[p0 + q].tolist()
                assert np.array_equal(xy[2 * v0:2 * (v0 + nv)], np.asarray(part, np.float64))
            k += 1
        wy, wx = C.ramp_tables((h, w), rec[1])
        wx = wx[::-1] if rec[2] else wx
        assert np.array_equal(src[b * 32:(b + 1) * 32], wy[rec[3][0]:rec[3][0] + 32])
        assert np.array_equal(src[3 * 32 + b * 32:3 * 32 + (b + 1) * 32], wx[rec[3][1]:rec[3][1] + 32])
    assert poly[:, 4].tolist() == (np.cumsum(poly[:, 5]) - poly[:, 5]).tolist() and lay["words"] == int(poly[:, 5].sum())
    # batch 1 is not cropped: the sample keeps its resized size
    one = COCO(_args(tree, batch_size=1), split="val", imsize=32)
    im, rec = one.host_item(1, random.Random(0))
    assert one.crop is False and rec == (1, (48, 32), False, None) and im.shape == (3, 48, 32)


def test_flags_parse():
    from rsis_amd.args import get_parser
    a = get_parser().parse_args(["-dataset", "coco", "-coco_dir", "/x", "-coco_val_set", "val2014"])
    assert (a.dataset, a.coco_dir, a.coco_train_set, a.coco_val_set) == ("coco", "/x", "train2017", "val2014")
    assert get_parser().parse_args([]).dataset == "pascal"


def test_header_library_and_binding_carry_the_symbol():
    from rsis_amd import _lib
    name = "rsis_paint_instance_maps"
    assert name + "(" in open(os.path.join(ROOT, "include", "rsis_hip.h")).read()
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 15
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert "cocomaps.hip" in open(os.path.join(ROOT, "rsis_amd", "csrc", "Makefile")).read()
