"""What DeviceLoader (rsis_amd/dataloader/loader.py) must yield, rebuilt outside it for any run of batches: the loader's per-sample
seeds replayed, `host_item` on the host, the label maps of the reader's kind (Cityscapes and COCO: the numpy statements of
tests/cityscapes_reader_cases.py and tests/coco_reader_cases.py), the matrices drawn from python's global stream in batch order, the
same warp, and sequence_from_masks of the warped maps.  Every comparison is exact."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cityscapes_reader_cases as CS  # noqa: E402
import coco_reader_cases as CC  # noqa: E402


def host_labels(kind, ds, index, item, sample_seed, annotation=None):
    """(ins, seg) of one sample at the output size, before the warp; `item` = ds.host_item(index, random.Random(sample_seed))"""
    if kind == "leaves":
        return item[1], (item[1] > 0).astype(np.int64)
    if kind == "pascal":
        return item[1], item[2]
    if kind == "cityscapes":                                   # the reference's full-resolution procedure -> zoom of both -> flip
        assert ds.crop is False
        size = item[0].shape[1:]
        ins, seg = CS.reference_raw_sample(ds.raw_ids(index))
        ins, seg = CS.zoom_nearest(ins, size), CS.zoom_nearest(seg, size)
        if ds.flip and random.Random(sample_seed).random() < 0.5:       # host_item's first draw
            ins, seg = ins[:, ::-1], seg[:, ::-1]
        return np.ascontiguousarray(ins), np.ascontiguousarray(seg)
    if kind == "coco":                                         # compose at native size -> zoom of both -> flip -> crop
        _index, resized, flip, crop = item[1]
        return CC.host_maps(annotation, ds.image_ids[index], resized, flip, crop, ds.imsize)
    raise ValueError(kind)


def expected_batches(kind, ds, batches, seed, matrix_seed, T, annotation=None):
    """[(x on the device, y_mask, y_class, sw_mask, sw_class as numpy)] for `batches`: the index lists of rank 0, in the order the
    loader stages them, over every epoch since its construction with `seed`; the global stream was seeded with `matrix_seed` before
    the first.  Call it after the loader has run: it fills the dataset's decode cache."""
    from rsis_amd.dataloader import sequence_from_masks
    from rsis_amd.dataloader.augment import affine_nearest
    from rsis_amd.dataloader.loader import MEAN, STD
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    rng = random.Random(seed * 1000003 + 1)                    # the loader's per-sample stream of rank 0
    random.seed(matrix_seed)                                   # RandomAffine draws from python's global stream, as the reference does
    out = []
    for idxs in batches:
        seeds = [rng.getrandbits(32) for _ in idxs]
        items = [ds.host_item(i, random.Random(s)) for i, s in zip(idxs, seeds)]
        labels = [host_labels(kind, ds, i, it, s, annotation) for i, it, s in zip(idxs, items, seeds)]
        H, W = items[0][0].shape[1:]
        x = (torch.from_numpy(np.stack([it[0] for it in items])).cuda().float() / 255.0 - mean) / std
        maps = [np.stack([lab[k] for lab in labels]) for k in (0, 1)]
        if ds.augmentation_transform is not None:
            mats = torch.stack([ds.augmentation_transform.matrix(H, W) for _ in idxs])
            x = affine_nearest(x, mats)
            maps = [affine_nearest(torch.from_numpy(m.astype(np.int64)).cuda().float().unsqueeze(1), mats).squeeze(1).round().long()
                    .cpu().numpy() for m in maps]
        t = np.stack([sequence_from_masks(i, s, T) for i, s in zip(*maps)])
        out.append((x, t[:, :, :-3].astype(np.float32), t[:, :, -3].astype(np.int64), t[:, :, -2].astype(np.float32),
                    t[:, :, -1].astype(np.float32)))
    return out


def assert_batch_equal(got, want):
    """got: one batch of the loader; want: one entry of expected_batches"""
    assert got[0].shape == want[0].shape and torch.equal(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
