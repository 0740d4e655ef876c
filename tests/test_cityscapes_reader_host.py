"""CPU tests of the Cityscapes reader (rsis_amd/dataloader/cityscapes.py): the commutation its host / device split rests on (numpy
statements in tests/cityscapes_reader_cases.py), get_raw_sample against the reference's full-resolution procedure, the file pairing,
and the shapes / flip of host_item.  Every comparison is exact."""
import argparse
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cityscapes_reader_cases as C  # noqa: E402


def _args(d, **kw):
    a = argparse.Namespace(gt_maxseqlen=20, batch_size=3, cityscapes_dir=d, rotation=10, translation=0.1, shear=0.1, zoom=0.7, crop=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from rsis_amd.dataloader.cityscapes import synthesize_cityscapes_dir
    return synthesize_cityscapes_dir(str(tmp_path_factory.mktemp("cs") / "CityScapes"), n=4, sizes=((64, 128), (50, 100)), seed=3)


def test_table_and_classes():
    from rsis_amd.dataloader import cityscapes as R
    assert list(R.CLASS_OF_LABEL) == C.TABLE and len(R.CLASS_OF_LABEL) == 34
    assert {l: c for l, c in enumerate(R.CLASS_OF_LABEL) if c} == {24: 1, 25: 2, 26: 3, 27: 4, 28: 5, 31: 6, 32: 7, 33: 8}
    assert R.CLASSES == ["<eos>", "person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
    # the table IS the reference's label arithmetic on every value the dataset can hold
    raw = np.array([[lab * 1000 + k for k in (0, 1, 999)] for lab in range(24, 34)] + [[0, 7, 999]])
    ins, seg = C.reference_raw_sample(raw)
    assert np.array_equal(seg, C.device_rule(raw)[1])
    assert np.array_equal(ins > 0, C.device_rule(raw)[0] > 0)


@pytest.mark.parametrize("full,small", C.COMMUTE_SIZES, ids=["64x128-16x32", "64x128-24x48", "96x200-25x52"])
def test_compaction_and_class_map_commute_with_nearest_sampling(full, small):
    """sequence_from_masks of (reference compaction at full size -> zoom of both maps) == of (zoom of the raw ids -> device rule)"""
    lost = 0
    for seed in (1, 2):
        raw = C.id_image(full[0], full[1], seed)
        assert set(np.unique(raw // 1000).tolist()) >= set(C.LABELS) and 26 in raw and (raw == 24900).sum() == (raw == 33900).sum() > 0
        ok, n_full, n_small = C.commutation_holds(raw, small)
        assert ok
        lost += n_full - n_small
    assert lost > 0                                            # some instance vanished under the sampling
    ok, n_full, n_small = C.commutation_holds(C.id_image(full[0], full[1], 3, background=False), small)
    assert ok and n_full == 19 and n_small == 20               # (no unmasked pixel: the reference's smallest instance is its rank 0)


def test_file_pairing_and_sorted_order(tree):
    from rsis_amd.dataloader.cityscapes import CityScapes
    for split in ("train", "val", "test"):
        ds = CityScapes(_args(tree), split=split)
        files = ds.get_sample_list()
        assert len(ds) == len(files) == 4 and files == sorted(files)
        assert [os.path.basename(os.path.dirname(f)) for f in files] == ["aachen", "aachen", "bochum", "bochum"]
        for f, g in zip(files, ds.ins_files):
            assert ("/leftImg8bit/%s/" % split) in f and f.endswith("_leftImg8bit.png")
            assert g == f.replace("/leftImg8bit/", "/gtFine/").replace("_leftImg8bit.png", "_gtFine_instanceIds.png") and os.path.exists(g)
            assert os.path.exists(g.replace("_instanceIds", "_labelIds"))
    assert ds.get_classes()[1] == "person" and ds.num_classes == 9 and ds.max_seq_len == 20


def test_synthesized_tree_is_what_it_claims(tree):
    from PIL import Image
    from rsis_amd.dataloader.cityscapes import CityScapes
    ds = CityScapes(_args(tree), split="train")
    labels, sizes = set(), set()
    for i in range(len(ds)):
        with Image.open(ds.ins_files[i]) as im:
            assert im.mode.startswith("I;16")
            raw = np.array(im).astype(np.int64)
        with Image.open(ds.ins_files[i].replace("_instanceIds", "_labelIds")) as im:
            assert im.mode == "L" and np.array_equal(np.array(im), np.where(raw >= 1000, raw // 1000, raw))
        assert ds.raw_size(i) == raw.shape and np.array_equal(ds.raw_ids(i), raw)
        sizes.add(raw.shape)
        inst = np.unique(raw[raw >= 1000])
        labels |= set((inst // 1000).tolist())
        assert 26 in raw and 7 in raw and len(inst) >= 6 and np.array_equal(raw, C.defined_for_reference(raw))
        assert any(k > 0 for k in (inst % 1000).tolist())      # several instances of one label
    assert labels == set(C.LABELS) and sizes == {(64, 128), (50, 100)}
    raw0 = ds.raw_ids(sorted(range(len(ds)), key=lambda i: ds.image_files[i])[0])
    assert (raw0 == 24000).sum() == (raw0 == 24001).sum() > 0  # the pair of equal area


def test_get_raw_sample_equals_the_reference_procedure(tree):
    from rsis_amd.dataloader.cityscapes import CityScapes
    ds = CityScapes(_args(tree), split="val")
    for i in range(len(ds)):
        img, ins, seg = ds.get_raw_sample(i)
        want_ins, want_seg = C.reference_raw_sample(ds.raw_ids(i))
        assert img.mode == "RGB" and img.size == ds.raw_size(i)[::-1]
        assert np.array_equal(ins, want_ins) and np.array_equal(seg, want_seg) and ins.max() >= 4
        assert set(np.unique(seg).tolist()) <= set(range(9))
    full = C.id_image(64, 128, 3, background=False)            # no unmasked pixel at all
    ds.raw_ids = lambda index: full
    _img, ins, seg = ds.get_raw_sample(0)
    want_ins, want_seg = C.reference_raw_sample(full)
    assert np.array_equal(ins, want_ins) and np.array_equal(seg, want_seg) and (ins == 0).any() and (seg > 0).all()


def test_host_item_shapes(tree):
    from PIL import Image
    from rsis_amd.dataloader.cityscapes import CityScapes
    rng = random.Random(0)
    ds = CityScapes(_args(tree), split="train", imsize=32)
    assert ds.crop is False and ds.same_size is True and ds.augmentation_transform is None
    shapes = set()
    for i in range(len(ds)):                                   # 64 x 128 and 50 x 100 originals -> 32 x 64
        im, ids = ds.host_item(i, rng)
        assert im.dtype == np.uint8 and im.shape == (3, 32, 64) and ids.dtype == np.int32 and ids.shape == (32, 64)
        shapes.add(ds.raw_size(i))
        with Image.open(ds.image_files[i]) as f:               # the image is PIL's BILINEAR resize, the ids one nearest zoom of the raw file
            assert np.array_equal(im, np.asarray(f.convert("RGB").resize((64, 32), Image.BILINEAR)).transpose(2, 0, 1))
        assert np.array_equal(ids, C.zoom_nearest(ds.raw_ids(i), (32, 64)))
        assert i in ds._cache
    assert shapes == {(64, 128), (50, 100)}
    ds = CityScapes(_args(tree), split="train", imsize=32, resize=True, augment=True)
    assert ds.augmentation_transform.zoom_range == (0.7, 1)
    im, ids = ds.host_item(0, rng)
    assert im.shape == (3, 32, 32) and ids.shape == (32, 32)
    ds = CityScapes(_args(tree, crop=True), split="train", imsize=32, augment=True)
    assert ds.crop is True and ds.augmentation_transform.zoom_range is None
    im, ids = ds.host_item(0, rng)
    assert im.shape == (3, 32, 32) and ids.shape == (32, 32)


def test_flip_flips_image_and_ids_together(tree):
    from rsis_amd.dataloader.cityscapes import CityScapes
    plain = CityScapes(_args(tree), split="train", imsize=32)
    aug = CityScapes(_args(tree), split="train", imsize=32, augment=True)
    assert aug.flip is True and plain.flip is False
    im0, ids0 = plain.host_item(1, random.Random(0))
    seen = set()
    for seed in range(8):
        flipped = random.Random(seed).random() < 0.5           # host_item's first draw
        im, ids = aug.host_item(1, random.Random(seed))
        if flipped:
            assert np.array_equal(im, im0[:, :, ::-1]) and np.array_equal(ids, ids0[:, ::-1]) and not np.array_equal(ids, ids0)
        else:
            assert np.array_equal(im, im0) and np.array_equal(ids, ids0)
        seen.add(flipped)
    assert seen == {True, False}


def test_loader_batches_same_size_datasets_without_crop_only(tree):
    from rsis_amd.dataloader.cityscapes import CityScapes
    from rsis_amd.dataloader.loader import DeviceLoader

    class Other(object):
        crop = False
        same_size = False
    with pytest.raises(ValueError):
        DeviceLoader(Other(), 3, device="cpu")
    dl = DeviceLoader(CityScapes(_args(tree), split="train", imsize=32), 3, device="cpu")
    assert len(dl) == 1
