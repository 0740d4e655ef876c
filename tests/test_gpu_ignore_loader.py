"""Where the ignore map comes from (--ignore_regions): the COCO reader's crowd records through rsis_rle_to_bits / rsis_poly_to_bits /
rsis_paint_ignore_map, the Cityscapes reader's group ids, and the DeviceLoader's sixth tensor -- each EQUAL to the numpy statement of
ignore_map_cases.py.  With the flag off the loaders yield 5-tuples, and the first five tensors do not depend on the flag."""
import argparse
import json
import os
import random

import numpy as np
import pytest
import torch

import coco_reader_cases as CR
import ignore_map_cases as M

pytestmark = pytest.mark.gpu
S = 32


def _coco_args(d, **kw):
    a = argparse.Namespace(gt_maxseqlen=20, batch_size=3, coco_dir=d, coco_train_set="train2017", coco_val_set="val2017", num_classes=4,
                           rotation=10, translation=0.1, shear=0.1, zoom=0.7, crop=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _city_args(d, **kw):
    a = argparse.Namespace(gt_maxseqlen=20, batch_size=3, cityscapes_dir=d, rotation=10, translation=0.1, shear=0.1, zoom=0.7, crop=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.fixture(scope="module")
def coco_tree(tmp_path_factory):
    from rsis_amd.dataloader.coco import synthesize_coco_dir
    return synthesize_coco_dir(str(tmp_path_factory.mktemp("coco_ign") / "COCO"), n=4, sizes=((48, 64), (75, 50), (33, 47)), seed=6)


@pytest.fixture(scope="module")
def hand_tree(tmp_path_factory):
    """two images, annotations only (the reader-level calls below never open an image): image 11 (40 x 56) has an outlined rectangle, a
    POLYGON crowd that overlaps it and reaches the right edge, and a run-count crowd in the lower left; image 12 (30 x 30) has an
    instance and no crowd"""
    from rsis_amd.dataloader.coco import _runs
    d = str(tmp_path_factory.mktemp("coco_hand") / "COCO")
    os.makedirs(os.path.join(d, "annotations"))
    m = np.zeros((40, 56), np.uint8)
    m[28:38, 2:14] = 1
    rect = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]      # noqa: E731
    anns = [dict(id=1, image_id=11, category_id=3, iscrowd=0, area=320.0, bbox=[10, 8, 20, 16], segmentation=[rect(10.0, 8.0, 30.0, 24.0)]),
            dict(id=2, image_id=11, category_id=3, iscrowd=1, area=900.0, bbox=[20, 4, 36, 26], segmentation=[rect(20.5, 4.0, 56.0, 30.25)]),
            dict(id=3, image_id=11, category_id=17, iscrowd=1, area=120.0, bbox=[2, 28, 12, 10], segmentation=dict(size=[40, 56], counts=_runs(m))),
            dict(id=4, image_id=12, category_id=17, iscrowd=0, area=100.0, bbox=[5, 5, 10, 10], segmentation=[rect(5.0, 5.0, 15.0, 15.0)])]
    with open(os.path.join(d, "annotations", "instances_train2017.json"), "w") as f:
        json.dump(dict(images=[dict(id=11, file_name="a.jpg", height=40, width=56), dict(id=12, file_name="b.jpg", height=30, width=30)],
                       annotations=anns, categories=[dict(id=3, name="car"), dict(id=17, name="cat")]), f)
    return d


def _annotation(tree):
    with open(os.path.join(tree, "annotations", "instances_train2017.json")) as f:
        return json.load(f)


def _resized(hw):
    h, w = hw
    return (S, max(S, int(S * w / h))) if w > h else (max(S, int(S * h / w)), S)


def _reader_maps(ds, records, mats=None):
    """what DeviceLoader does with a staged batch, for hand-picked records: table -> device -> maps_to_warp -> the shared warp ->
    (ins, ignore map)"""
    from rsis_amd.dataloader.augment import affine_nearest
    table, layout = ds.stage_tables(records, (S, S))
    maps = ds.maps_to_warp([], torch.from_numpy(table).cuda(), layout)
    warped = []
    for m in maps:
        mf = m.float().unsqueeze(1)
        if mats is not None:
            mf = affine_nearest(mf, mats)
        warped.append(mf.squeeze(1).round().long())
    ins, _seg = ds.label_maps(warped)
    return ins.cpu().numpy(), ds.ignore_map(warped)


def _want(ds, ann, records, mats=None):
    from rsis_amd.dataloader.augment import affine_nearest
    from rsis_amd.dataloader.coco import index_tables
    out = []
    for index, resized, flip, crop in records:
        sy, sx = index_tables(ds.raw_size(index), resized, flip, crop, (S, S))
        ins, _seg = CR.host_maps(ann, ds.image_ids[index], resized, flip, crop, S)
        out.append(M.coco_ignore(ann, ds.image_ids[index], sy, sx, ins))
    out = np.stack(out)
    if mats is not None:
        out = affine_nearest(torch.from_numpy(out).cuda().float().unsqueeze(1), mats).squeeze(1).round().long().cpu().numpy().astype(np.uint8)
    return out


def _records(ds, kind):
    recs = []
    for i in range(min(3, len(ds))):
        rh, rw = _resized(ds.raw_size(i))
        if kind == "resize":
            recs.append((i, (S, S), False, None))
        else:                                                   # flip + crop, offsets inside the resized image
            recs.append((i, (rh, rw), True, ((rh - S) // 3, (rw - S) // 2)))
    return recs


@pytest.mark.parametrize("kind", ["resize", "flip_crop", "augment"])
@pytest.mark.parametrize("which", ["synthetic", "hand"])
def test_coco_ignore_map_equals_the_numpy_statement(coco_tree, hand_tree, which, kind):
    from rsis_amd.dataloader.coco import COCO
    tree = coco_tree if which == "synthetic" else hand_tree
    ann = _annotation(tree)
    ds = COCO(_coco_args(tree, ignore_regions=True, num_classes=4 if which == "synthetic" else 3), split="train", imsize=S, augment=kind == "augment")
    if which == "synthetic":        # image 0 carries a crowd as run counts; the image with only a crowd and the empty one are left out
        assert len(ds) == 4 and [len(c) for c in ds.crowds] == [1, 0, 0, 0] and ds.crowds[0][0][0] == "counts"
    else:
        assert len(ds) == 2 and [[k for k, _d in c] for c in ds.crowds] == [["polygons", "counts"], []]
    mats = None
    records = _records(ds, "flip_crop" if kind == "augment" else kind)
    if kind == "augment":
        random.seed(11)
        mats = torch.stack([ds.augmentation_transform.matrix(S, S) for _ in records])
    ins, got = _reader_maps(ds, records, mats)
    want = _want(ds, ann, records, mats)
    got = (got != 0).cpu().numpy().astype(np.uint8)
    assert got.shape == want.shape == (len(records), S, S)
    assert np.array_equal(got, want)
    assert all(want[b].sum() == 0 for b in range(1, len(records)))
    assert not (got.astype(bool) & (ins > 0)).any()            # an outlined instance inside a crowd still counts
    if kind != "augment":
        # the crowd of sample 0 before the "clear where painted" step: it overlaps painted instances (the synthetic writer's crowd lies
        # wholly inside them: its map is empty BECAUSE of the rule; the hand-made polygon crowd reaches past its instance and stays)
        from rsis_amd.dataloader.coco import index_tables
        sy, sx = index_tables(ds.raw_size(0), *records[0][1:], (S, S))
        raw = M.coco_ignore(ann, ds.image_ids[0], sy, sx, np.zeros((S, S), np.int32))
        assert raw.sum() > 0 and (raw.astype(bool) & (ins[0] > 0)).any()
    if which == "hand":
        assert want[0].sum() > 0


def _write_images(tree):
    """the hand-made tree gets its two JPEG files, so that a DeviceLoader can run on it"""
    from PIL import Image
    os.makedirs(os.path.join(tree, "train2017"), exist_ok=True)
    for name, (h, w) in (("a.jpg", (40, 56)), ("b.jpg", (30, 30))):
        Image.fromarray(np.random.default_rng(h).integers(0, 255, (h, w, 3)).astype(np.uint8)).save(os.path.join(tree, "train2017", name))


def test_coco_loader_yields_the_map_only_with_the_flag(hand_tree):
    """batch 2 of the hand-made file through DeviceLoader: 6-tuple with the (B, N) uint8 contiguous map, equal to the statement for the
    loader's own draws (no flip without --augment; the crop offsets of its per-sample stream); 5-tuple, same five tensors, without"""
    from rsis_amd.dataloader.coco import COCO
    from rsis_amd.dataloader.loader import DeviceLoader
    _write_images(hand_tree)
    ann = _annotation(hand_tree)
    seed = 5
    batches = []
    for flag in (True, False):
        ds = COCO(_coco_args(hand_tree, ignore_regions=flag, num_classes=3, batch_size=2), split="train", imsize=S, augment=False)
        batches.append(next(iter(DeviceLoader(ds, 2, shuffle=False, num_workers=2, seed=seed))))
    torch.cuda.synchronize()
    with_map, without = batches
    assert len(with_map) == 6 and len(without) == 5
    assert all(torch.equal(p, q) for p, q in zip(with_map[:5], without))
    ign = with_map[5]
    assert ign.dtype == torch.uint8 and tuple(ign.shape) == (2, S * S) and ign.is_contiguous() and ign.is_cuda
    rng = random.Random(seed * 1000003 + 1)
    records = []
    for i in range(2):
        r = random.Random(rng.getrandbits(32))
        rh, rw = _resized(ds.raw_size(i))
        ow = 0 if (rw - S) // 2 <= 0 else r.randrange((rw - S) // 2)
        oh = 0 if (rh - S) // 2 <= 0 else r.randrange((rh - S) // 2)
        records.append((i, (rh, rw), False, (oh, ow)))
    want = _want(ds, ann, records)
    assert np.array_equal(ign.cpu().numpy().reshape(2, S, S), want) and want[0].sum() > 0
    # y_mask is zero under the map: a crowd pixel with no painted instance belongs to no ground-truth mask
    assert float((with_map[1] * ign.unsqueeze(1).float()).sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------- Cityscapes
@pytest.fixture(scope="module")
def city_tree(tmp_path_factory):
    """the synthetic tree, its train id images overwritten with bands on the left: "person group" 24, "car group" 26, "caravan group" 29
    (not trained), void ids 3 and 0, next to the instances and stuff the writer drew"""
    from PIL import Image
    from rsis_amd.dataloader.cityscapes import synthesize_cityscapes_dir
    d = synthesize_cityscapes_dir(str(tmp_path_factory.mktemp("cs_ign") / "CityScapes"), n=4, sizes=((64, 128),), seed=6)
    import glob
    for f in sorted(glob.glob(os.path.join(d, "gtFine", "train", "*", "*_gtFine_instanceIds.png"))):
        with Image.open(f) as im:
            ids = np.array(im).astype(np.uint16)
        for k, v in enumerate((24, 26, 29, 3, 0)):
            ids[12 * k:12 * k + 10, 2:22] = v
        Image.fromarray(ids).save(f)
    return d


def test_cityscapes_ignore_map_after_the_warp(city_tree):
    """augmentation on, batch 3 of un-cropped 32 x 64 samples: the sixth tensor equals the rule applied to the warped raw ids (zoom ->
    flip -> the same warp), and the first five tensors are those of the loader without the flag"""
    from rsis_amd.dataloader.augment import affine_nearest
    from rsis_amd.dataloader.cityscapes import CLASS_OF_LABEL, CityScapes
    from rsis_amd.dataloader.loader import DeviceLoader
    from rsis_amd.dataloader.reader import zoom_map
    H, W = 32, 64
    batches = []
    for flag in (True, False):
        ds = CityScapes(_city_args(city_tree, ignore_regions=flag), split="train", imsize=32, augment=True)
        random.seed(11)                                       # RandomAffine draws from python's global stream
        batches.append(next(iter(DeviceLoader(ds, 3, shuffle=False, num_workers=2, seed=5))))
    torch.cuda.synchronize()
    with_map, without = batches
    assert len(with_map) == 6 and len(without) == 5
    assert all(torch.equal(p, q) for p, q in zip(with_map[:5], without))          # x, and through the targets ins and seg: unchanged
    ign = with_map[5]
    assert ign.dtype == torch.uint8 and tuple(ign.shape) == (3, H * W) and ign.is_contiguous()
    rng = random.Random(5 * 1000003 + 1)
    flips = [random.Random(rng.getrandbits(32)).random() < 0.5 for _ in range(3)]
    random.seed(11)
    mats = torch.stack([ds.augmentation_transform.matrix(H, W) for _ in range(3)])
    raws = []
    for i, f in enumerate(flips):
        raw = zoom_map(ds.raw_ids(i), (H, W))
        raws.append(np.ascontiguousarray(raw[:, ::-1] if f else raw))
    warped = affine_nearest(torch.from_numpy(np.stack(raws)).cuda().float().unsqueeze(1), mats).squeeze(1).round().long().cpu().numpy()
    want = M.cityscapes_ignore(warped, CLASS_OF_LABEL)
    assert np.array_equal(ign.cpu().numpy().reshape(3, H, W).astype(bool), want)
    # groups of trained classes are in the map; the untrained group, the void bands and the warp's zero fill are not
    assert want.sum() > 0 and set(np.unique(warped[want]).tolist()) <= {24, 25, 26, 27, 28, 31, 32, 33} and {24, 26} <= set(np.unique(warped[want]).tolist())
    assert (warped == 29).any() and not want[warped == 29].any() and not want[warped == 0].any() and not want[warped == 3].any()
    assert any(not np.array_equal(warped[b], raws[b]) for b in range(3))
    # the reader-level rule, on ids it never saw on a file: instance ids, a group beyond the table
    ids = torch.tensor([[[24000, 26001, 24, 26, 29, 33, 34, 999, 1000, 0]]], device="cuda")
    ds_on = CityScapes(_city_args(city_tree, ignore_regions=True), split="train", imsize=32)
    assert ds_on.ignore_map([ids]).cpu().numpy().tolist() == [[[False, False, True, True, False, True, False, False, False, False]]]
    assert ds.ignore_map([ids]) is None
