"""Pascal VOC, host side (rsis_amd/dataloader/pascal.py, rsis_amd/pascal_precompute.py, the ground-truth file reader of rsis_amd.eval):
the colour table, the numpy statement of the preparation, the ground-truth records, the dataset surface and the pickle flavours.
The device side is tests/test_gpu_pascal.py."""
import argparse
import os
import pickle
import random

import numpy as np
import pytest


def _args(d, **kw):
    a = argparse.Namespace(gt_maxseqlen=10, batch_size=4, pascal_dir=d, rotation=10, translation=0.1, shear=0.1, zoom=0.7)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def rle_numpy(mask):
    """run counts of a binary (h, w) mask in column-major order, starting with the run of zeros (maskApi.c rleEncode)"""
    v = np.asarray(mask, np.uint8).T.reshape(-1)
    pos = np.flatnonzero(np.diff(np.concatenate([[0], v]))).tolist()
    return np.diff([0] + pos + [v.size]).astype(np.uint32)


def numpy_encoder(idmap, ids):
    """the `encode` argument of make_records without the device: numpy run counts, text by the library's host function"""
    from rsis_amd.cocoeval import rle_to_string
    return [rle_to_string(rle_numpy(np.asarray(idmap) == i)) for i in ids]


def decode(seg):
    from rsis_amd.cocoeval import rle_from_string
    h, w = seg["size"]
    c = rle_from_string(seg["counts"])
    return np.repeat(np.arange(len(c)) & 1, c.astype(np.int64)).reshape(w, h).T.astype(np.uint8)


def precompute_tree_numpy(d, splits=("train", "val")):
    """ProcMasks of a synthesized tree from the numpy statement (what the device preparation must equal)"""
    from PIL import Image
    from rsis_amd.pascal_precompute import get_imnames, precompute_numpy
    os.makedirs(os.path.join(d, "ProcMasks"), exist_ok=True)
    out = {}
    for split in splits:
        for name in get_imnames(d, split):
            cla = np.asarray(Image.open(os.path.join(d, "SegmentationClass", name + ".png")).convert("RGB"))
            obj = np.asarray(Image.open(os.path.join(d, "SegmentationObject", name + ".png")).convert("RGB"))
            masks, ignore = precompute_numpy(cla, obj)
            np.save(os.path.join(d, "ProcMasks", name + ".npy"), masks)
            out[name] = (masks, ignore)
    return out


def test_palette_table_is_the_voc_bit_interleave():
    from rsis_amd.dataloader.pascal import CLASSES, palette_table, voc_colormap
    from rsis_amd.pascal_precompute import ids_from_colors_numpy
    t = palette_table()
    assert t.shape == (22, 4) and t.dtype == np.uint8 and len(CLASSES) == 21 and CLASSES[0] == "<eos>"
    for row in t:                                             # the formula, bit by bit
        i = int(row[3])
        want = [sum(((i >> (3 * j + ch)) & 1) << (7 - j) for j in range(3)) for ch in range(3)]
        assert [int(v) for v in row[:3]] == want
    # well-known entries of the VOC colour map
    assert tuple(t[0]) == (0, 0, 0, 0) and tuple(t[1]) == (128, 0, 0, 1) and tuple(t[15]) == (192, 128, 128, 15)
    assert tuple(t[20]) == (0, 64, 128, 20) and tuple(t[21]) == (224, 224, 192, 255)
    assert [int(v) for v in t[:, 3]] == list(range(21)) + [255]
    cm = voc_colormap()
    px = np.array([[cm[0], cm[20], (224, 224, 192), (1, 2, 3), cm[21], cm[7]]], np.uint8)      # void, an unknown colour, object id 21
    assert ids_from_colors_numpy(px).tolist() == [[0, 20, 255, 0, 0, 7]]


def test_precompute_numpy_on_a_hand_example():
    from rsis_amd.dataloader.pascal import voc_colormap
    from rsis_amd.pascal_precompute import precompute_numpy
    cm = voc_colormap()
    V = 255
    seg = np.zeros((7, 9), np.int64)
    ins = np.zeros((7, 9), np.int64)
    seg[1:4, 1:4], ins[1:4, 1:4] = 15, 1
    seg[1:4, 5:8], ins[1:4, 5:8] = 15, 2
    seg[5, 1:8], ins[5, 1:8] = 7, 22                          # an object id above 20: falls to background
    seg[4, :] = V                                             # a void line in the class map only
    ins[0, 0] = V                                             # void in the object map alone is NOT an ignore pixel: it stays 255
    assert tuple(cm[255]) == (224, 224, 192)                  # the void colour IS entry 255 of the colour map
    col = cm
    masks, ignore = precompute_numpy(col[seg], col[ins])
    assert masks.shape == (7, 9, 2) and masks.dtype == np.uint8 and ignore.dtype == np.uint8
    want_seg, want_ins = seg.copy(), ins.copy()
    want_ins[ins == 22] = 0
    want_seg[4, :] = 0
    assert np.array_equal(ignore, (seg == V).astype(np.uint8)) and int(ignore.sum()) == 9
    assert np.array_equal(masks[:, :, 0], want_seg) and np.array_equal(masks[:, :, 1], want_ins)


def test_records_ascending_ids_then_twenty_ignore_records():
    from rsis_amd.dataloader.pascal import CLASSES
    from rsis_amd.pascal_precompute import make_records
    seg = np.zeros((7, 9), np.uint8)
    ins = np.zeros((7, 9), np.uint8)
    ins[0:2, 0:3], seg[0:2, 0:3] = 5, 12
    ins[3:6, 2:8], seg[3:6, 2:8] = 2, 9
    seg[3, 2:4] = 4                                           # an instance over two classes: the smaller class id names it
    ins[6, 8], seg[6, 8] = 9, 20
    for ignore in (np.zeros((7, 9), np.uint8), (np.arange(63).reshape(7, 9) % 5 == 0).astype(np.uint8)):
        recs = make_records("2007_000001\n", np.stack([seg, ins], -1), ignore, numpy_encoder)
        assert len(recs) == 3 + 20                            # the ignore records are there even for an empty ignore mask
        assert [r["category_id"] for r in recs[:3]] == [4, 12, 20] and [r["ignore"] for r in recs] == [0] * 3 + [1] * 20
        assert [r["category_id"] for r in recs[3:]] == list(range(1, 21))
        assert all(r["image_id"] == "2007_000001" and r["score"] == 1 and r["category_name"] == CLASSES[r["category_id"]] for r in recs)
        assert all(type(r["category_id"]) is int and r["segmentation"]["size"] == [7, 9] for r in recs)
        for r, i in zip(recs[:3], (2, 5, 9)):
            assert np.array_equal(decode(r["segmentation"]), (ins == i).astype(np.uint8))
        assert all(np.array_equal(decode(r["segmentation"]), ignore) for r in recs[3:])
    # an image without id 0: the smallest id present is the background (np.unique(ins)[1:])
    recs = make_records("x", np.stack([seg, np.where(ins == 0, 1, ins).astype(np.uint8)], -1), ignore, numpy_encoder)
    assert len(recs) == 3 + 20 and np.array_equal(decode(recs[0]["segmentation"]), (ins == 2).astype(np.uint8))


def test_synthesized_tree_and_dataset_surface(tmp_path):
    from rsis_amd.dataloader.pascal import PascalVOC, synthesize_pascal_dir
    d = synthesize_pascal_dir(str(tmp_path / "VOC"), n=6, sizes=((48, 64), (75, 50)), seed=4)
    # a split file in an order that is not sorted: the dataset keeps FILE order
    with open(os.path.join(d, "ImageSets", "Segmentation", "train.txt")) as f:
        names = f.read().split()
    assert len(names) == 4
    shuffled = [names[2], names[0], names[3], names[1]]
    with open(os.path.join(d, "ImageSets", "Segmentation", "train.txt"), "w") as f:
        f.write("".join(s + "\n" for s in shuffled))
    truth = precompute_tree_numpy(d)
    assert len(truth) == 6
    classes = set()
    for name, (masks, ignore) in truth.items():
        ids = np.unique(masks[:, :, 1])
        assert ids[0] == 0 and 2 <= len(ids) - 1 <= 7 and ignore.any()
        assert not (masks[:, :, 1][ignore > 0]).any() and not (masks[:, :, 0][ignore > 0]).any()
        classes |= set(np.unique(masks[:, :, 0]).tolist()) - {0}
    assert len(classes) >= 3
    first = truth[names[0]][0][:, :, 1]
    assert int((first == 1).sum()) == int((first == 2).sum()) > 0           # two instances of equal area
    tr = PascalVOC(_args(d), split="train", imsize=32)
    va = PascalVOC(_args(d, batch_size=1), split="val", imsize=32, augment=True)
    assert tr.get_sample_list() == shuffled and len(tr) == 4 and len(va) == 2
    assert tr.get_classes()[0] == "<eos>" and len(tr.get_classes()) == 21 and tr.num_classes == 21 and tr.max_seq_len == 10
    assert tr.image_dir == os.path.join(d, "JPEGImages") and tr.masks_dir == os.path.join(d, "ProcMasks")
    assert tr.crop is True and tr.flip is False and tr.augmentation_transform is None
    assert va.crop is False and va.flip is True
    assert va.augmentation_transform.zoom_range == (0.7, 1.4)               # (zoom, max(2 * zoom, 1)), --resize or not
    assert PascalVOC(_args(d, zoom=0.4), split="val", augment=True).augmentation_transform.zoom_range == (0.4, 1.0)
    img, ins, seg = tr.get_raw_sample(1)
    masks = truth[shuffled[1]][0]
    assert img.mode == "RGB" and img.size == (ins.shape[1], ins.shape[0]) and tr.raw_size(1) == ins.shape
    assert np.array_equal(ins, masks[:, :, 1]) and np.array_equal(seg, masks[:, :, 0])


def test_host_item_shapes_with_and_without_resize(tmp_path):
    from rsis_amd.dataloader.pascal import PascalVOC, synthesize_pascal_dir
    d = synthesize_pascal_dir(str(tmp_path / "VOC"), n=6, sizes=((48, 64), (75, 50)), seed=5)
    truth = precompute_tree_numpy(d)
    tr = PascalVOC(_args(d), split="train", imsize=32, augment=True)
    for i in range(len(tr)):
        im, ins, seg = tr.host_item(i, random.Random(i))
        assert im.shape == (3, 32, 32) and im.dtype == np.uint8
        assert ins.shape == seg.shape == (32, 32) and ins.dtype == seg.dtype == np.int32
        masks = truth[tr.get_sample_list()[i]][0]
        # nearest resize of both maps: no new ids, and class and instance still belong together
        assert set(np.unique(ins)) <= set(np.unique(masks[:, :, 1])) and set(np.unique(seg)) <= set(np.unique(masks[:, :, 0]))
        pairs = set(zip(masks[:, :, 1].reshape(-1).tolist(), masks[:, :, 0].reshape(-1).tolist()))
        assert set(zip(ins.reshape(-1).tolist(), seg.reshape(-1).tolist())) <= pairs
    sq = PascalVOC(_args(d), split="train", imsize=40, resize=True)
    im, ins, seg = sq.host_item(0, random.Random(0))
    assert im.shape == (3, 40, 40) and ins.shape == seg.shape == (40, 40)
    # batch_size 1: no crop, the shorter side goes to imsize
    one = PascalVOC(_args(d, batch_size=1), split="train", imsize=24)
    shapes = sorted(one.host_item(i, random.Random(0))[1].shape for i in range(len(one)))
    assert shapes == sorted([(24, 32), (36, 24), (24, 32), (36, 24)])
    # the decode cache holds all three arrays and counts their bytes
    assert len(sq._cache) == 1 and sq._cache_bytes == 3 * 40 * 40 + 2 * 40 * 40 * sq._cache[0][1].itemsize


def test_ground_truth_pickles_of_both_pythons_load_and_classes_are_refused(tmp_path):
    from rsis_amd.utils.utils import load_plain_pickle
    recs = [{"image_id": "2007_000033", "category_id": 3, "category_name": "bird", "segmentation": {"size": [7, 9], "counts": b"0o1"},
             "score": 1, "ignore": 0}]
    for proto in (2, pickle.HIGHEST_PROTOCOL):
        p = tmp_path / ("py3_%d.pkl" % proto)
        p.write_bytes(pickle.dumps(recs, protocol=proto))
        assert load_plain_pickle(str(p)) == recs
    # python 2, protocol 2: [{'counts': '0o1', 'image_id': 'caf\xe9'}] with str payloads as SHORT_BINSTRING ('U')
    py2 = b"\x80\x02]q\x00}q\x01(U\x06countsq\x02U\x030o1q\x03U\x08image_idq\x04U\x04caf\xe9q\x05ua."
    p = tmp_path / "py2.pkl"
    p.write_bytes(py2)
    got = load_plain_pickle(str(p))
    assert got == [{"counts": "0o1", "image_id": "café"}]
    # python 2, protocol 0 (what pickle.dump(obj, f) wrote there): the same through STRING opcodes
    p.write_bytes(b"(lp0\n(dp1\nS'counts'\np2\nS'0o1'\np3\nsa.")
    assert load_plain_pickle(str(p)) == [{"counts": "0o1"}]
    import collections
    bad = tmp_path / "bad.pkl"
    bad.write_bytes(pickle.dumps([collections.OrderedDict(a=1)], protocol=2))
    with pytest.raises(pickle.UnpicklingError):
        load_plain_pickle(str(bad))
    bad.write_bytes(b"cos\nsystem\n(S'true'\ntR.")
    with pytest.raises(pickle.UnpicklingError):
        load_plain_pickle(str(bad))


def test_rle_text_round_trip_of_the_numpy_encoder():
    """the helper the record tests lean on: its counts decode to the mask (so a wrong helper cannot hide a wrong record)"""
    r = np.random.default_rng(0)
    m = (r.random((7, 9)) < 0.4).astype(np.uint8)
    c = rle_numpy(m)
    assert int(c.sum()) == 63 and np.array_equal(np.repeat(np.arange(len(c)) & 1, c).reshape(9, 7).T, m)
    assert c.dtype == np.uint32
