"""DeviceLoader (rsis_amd/dataloader/loader.py) over EVERY batch of two epochs, for each of the four readers: 7 samples at a per-rank
batch of 3 without drop_last -- batches of 3, 3, 1 -- so that both pinned sets of both batch sizes are refilled under their events, the
second epoch runs from the decode cache, and the short last batch is staged twice.  Every batch equals tests/loader_expect.py bit for
bit."""
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loader_expect as E  # noqa: E402

S, T, SEED, MATRIX_SEED = 32, 10, 5, 11


def _leaves(root):
    from rsis_amd.dataloader.leaves import LeavesDataset, synthesize_leaves_dir
    from test_leaves_loader import _args
    d = synthesize_leaves_dir(os.path.join(root, "A1"), n=7, size=(96, 112), seed=2)
    return LeavesDataset(_args(d, batch_size=3, gt_maxseqlen=T), split="train", imsize=S, augment=True), None


def _pascal(root):
    from rsis_amd.dataloader.pascal import PascalVOC, synthesize_pascal_dir
    from test_pascal_host import _args, precompute_tree_numpy
    d = synthesize_pascal_dir(os.path.join(root, "VOC"), n=10, sizes=((48, 64), (75, 50)), seed=6)     # 7 train + 3 val
    precompute_tree_numpy(d, splits=("train",))
    return PascalVOC(_args(d, batch_size=3, gt_maxseqlen=T), split="train", imsize=S, augment=True), None


def _cityscapes(root):
    from rsis_amd.dataloader.cityscapes import CityScapes, synthesize_cityscapes_dir
    from test_cityscapes_reader_host import _args
    d = synthesize_cityscapes_dir(os.path.join(root, "CityScapes"), n=7, sizes=((64, 128),), seed=6)
    return CityScapes(_args(d, batch_size=3, gt_maxseqlen=T), split="train", imsize=S, augment=True), None


def _coco(root):
    from rsis_amd.dataloader.coco import COCO, synthesize_coco_dir
    from test_coco_reader_host import _args
    d = synthesize_coco_dir(os.path.join(root, "COCO"), n=7, sizes=((48, 64), (75, 50), (33, 47)), seed=6)
    with open(os.path.join(d, "annotations", "instances_train2017.json")) as f:
        annotation = json.load(f)
    return COCO(_args(d, batch_size=3, gt_maxseqlen=T), split="train", imsize=S, augment=True), annotation


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["leaves", "pascal", "cityscapes", "coco"])
def test_every_batch_of_two_epochs_equals_the_host_expectation(kind, tmp_path):
    from rsis_amd.dataloader.loader import DeviceLoader
    ds, annotation = {"leaves": _leaves, "pascal": _pascal, "cityscapes": _cityscapes, "coco": _coco}[kind](str(tmp_path))
    assert len(ds) == 7 and ds.augmentation_transform is not None and ds.crop is (kind != "cityscapes")
    dl = DeviceLoader(ds, 3, shuffle=False, num_workers=2, seed=SEED, drop_last=False)
    assert len(dl) == 3
    random.seed(MATRIX_SEED)
    first = list(dl)
    assert sorted(ds._cache) == list(range(7))                 # the second epoch runs from the decode cache
    got = first + list(dl)
    assert [b[0].size(0) for b in got] == [3, 3, 1, 3, 3, 1]
    want = E.expected_batches(kind, ds, [[0, 1, 2], [3, 4, 5], [6]] * 2, SEED, MATRIX_SEED, T, annotation)
    for g, w in zip(got, want):
        E.assert_batch_equal(g, w)
    assert any(w[2].any() for w in want) and got[0][1].shape == (3, T) + (got[0][0].size(-2) * got[0][0].size(-1),)
