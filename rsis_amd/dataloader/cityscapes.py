"""Cityscapes reader -- the reference's src/dataloader/cityscapes.py:9-94 on the base class of reader.py and the device loader of
loader.py:
  host   : the file list, PNG decode and the PIL bilinear `Scale` of the image, ONE nearest zoom of the RAW `*_gtFine_instanceIds.png`
           values to the image size; flip, the optional crop (`-crop`) and the decode cache are Reader's; `same_size`, so that
           un-cropped samples are batched;
  device : normalisation, one affine warp shared by the image and the raw id map, then `label_maps` = `maps_from_ids`: class map +
           compact instance map (rsis_instance_maps), and the targets (rsis_targets_from_maps).
The reference derives both maps at full resolution on the host (np.unique over 2 M pixels and one full-image compare per instance,
cityscapes.py:67-92) and resamples them afterwards.  The class of a pixel is a function of its raw id alone, and the compact instance
id is the rank of the raw id among the kept ids present -- order-preserving -- so both commute with every step that only MOVES
pixels (nearest zoom, flip, crop, the nearest affine warp; ids below 2^24 are exact in the warp's float32): sequence_from_masks of
the maps is the same either way, including instances that vanish under sampling (tests/cityscapes_reader_cases.py).
Deviations: the file list is sorted (the reference takes glob's order); a raw value >= 1000 of a label 1..23 --
which the dataset does not contain and for which the reference's unsigned arithmetic wraps -- is "not an instance" here."""
import glob
import os

import numpy as np
import torch

from .reader import Reader, scale_image, zoom_map

CLASSES = ["<eos>", "person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]       # cityscapes.py:20
# labelId -> class: cityscapes.py:68-80 under python-2 integer division (caravan 29 and trailer 30 are not trained)
CLASS_OF_LABEL = [0] * 24 + [1, 2, 3, 4, 5, 0, 0, 6, 7, 8]
INSTANCE_LABELS = (24, 25, 26, 27, 28, 29, 30, 31, 32, 33)

_TABLES = {}


def _table(device):
    """CLASS_OF_LABEL as an int32 tensor on `device`, made once per device"""
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = torch.tensor(CLASS_OF_LABEL, dtype=torch.int32, device=device)
    return _TABLES[key]


def maps_from_ids(ids, table=None):
    """(B, H, W) CUDA integer tensor of raw `instanceIds` values -> (ins, seg) int32 CUDA tensors: seg = the class 0..8 of every pixel,
    ins = 1 + the rank of the pixel's id among the distinct ids of its image that have a class, 0 elsewhere (rsis_instance_maps: two
    passes over the batch, no host sync).  `table`: another label -> class table (int32 CUDA tensor of at most 66 entries)."""
    from .._lib import check, lib, ptr, stream
    if not ids.is_cuda:
        raise RuntimeError("maps_from_ids runs in librsis_hip.so: a CUDA tensor is required (there is no CPU path)")
    L = lib()
    raw = ids.to(torch.int32).contiguous()
    B, H, W = raw.shape
    tab = _table(raw.device) if table is None else table.to(device=raw.device, dtype=torch.int32).contiguous()
    ins, seg = torch.empty_like(raw), torch.empty_like(raw)          # every element is written by the kernel
    if raw.numel() == 0:
        return ins, seg
    work = torch.empty((int(L.rsis_instance_maps_work_ints(B)),), dtype=torch.int32, device=raw.device)
    check(L.rsis_instance_maps(ptr(raw), ptr(tab), int(tab.numel()), B, H, W, ptr(ins), ptr(seg), ptr(work), stream()),
          "rsis_instance_maps")
    return ins, seg


def ignore_from_ids(ids, table=None):
    """(B, H, W) integer tensor of (warped) raw `instanceIds` values -> bool (B, H, W): the GROUP regions of trained classes, a bare
    labelId below 1000 whose class is not 0 ("person group" = 24, "car group" = 26).  Void labels, groups of untrained labels (caravan
    29, trailer 30) and the warp's zero fill stay counted as background.  A torch expression: once per batch, not hot."""
    tab = _table(ids.device) if table is None else table.to(device=ids.device, dtype=torch.int32)
    raw = ids.long()
    small = (raw >= 0) & (raw < tab.numel())                 # (tab has 34 entries: every index below 1000 that has a class)
    return small & (tab[raw.clamp(0, tab.numel() - 1)] > 0)


class CityScapes(Reader):
    """reference CityScapes(MyDataset): same constructor arguments, `classes`, `get_classes`, `get_sample_list`, `__len__`,
    `get_raw_sample`; `host_item` returns (image, RAW ids) and the loader calls `maps_from_ids` after the warp"""
    same_size = True            # every image of the dataset has one size (1024 x 2048): un-cropped samples can be batched
    has_ignore_source = True    # group regions: --ignore_regions

    def __init__(self, args, transform=None, target_transform=None, augment=False, split="train", resize=False, imsize=256):
        self._setup(args, transform, target_transform, augment, split, resize, imsize, crop=bool(args.crop),   # cityscapes.py:36-49
                    zoom_range=(args.zoom, 1) if resize else None)
        self.classes = list(CLASSES)
        self.num_classes = len(self.classes)
        self.image_files = sorted(glob.glob(os.path.join(args.cityscapes_dir, "leftImg8bit", split, "*", "*.png")))
        self.ins_files = [w.replace("/leftImg8bit/", "/gtFine/").replace("_leftImg8bit.png", "_gtFine_instanceIds.png")
                          for w in self.image_files]                        # cityscapes.py:26-27 (the labelIds files are never read)
        self.no_run_coco_eval = True

    maps_from_ids = staticmethod(maps_from_ids)

    def label_maps(self, maps):
        ids, = maps
        return self.maps_from_ids(ids)

    def ignore_map(self, maps):
        ids, = maps
        return ignore_from_ids(ids) if self.ignore_regions else None

    def raw_ids(self, index):
        """the `*_gtFine_instanceIds.png` of a sample as an int32 array"""
        from PIL import Image
        with Image.open(self.ins_files[index]) as im:
            return np.array(im).astype(np.int32)

    def get_raw_sample(self, index):
        """(PIL RGB image, instance-id map, class map) in raw size -- cityscapes.py:58-94: ids compacted to their rank among the unique
        values of the masked map (with no unmasked pixel at all, the smallest instance takes rank 0, as it does there).  API parity only:
        the loader works on the raw ids (module docstring)."""
        from PIL import Image
        img = Image.open(self.image_files[index]).convert("RGB")
        raw = self.raw_ids(index)
        table = np.asarray(CLASS_OF_LABEL, np.int32)
        label = raw // 1000
        seg = np.where((raw >= 1000) & (label < len(table)), table[np.clip(label, 0, len(table) - 1)], 0).astype(np.int32)
        _ids, rank = np.unique(np.where(seg > 0, raw, 0), return_inverse=True)
        return img, rank.reshape(raw.shape).astype(np.int32), seg

    def _decode(self, index):
        from PIL import Image
        im = scale_image(Image.open(self.image_files[index]).convert("RGB"), self.imsize, self.resize)
        return im, zoom_map(self.raw_ids(index), im.shape[1:])


def synthesize_cityscapes_dir(path, n=4, sizes=((64, 128),), cities=("aachen", "bochum"), seed=0):
    """Write a small Cityscapes-shaped tree with n images in each of the splits train / val / test:
    leftImg8bit/<split>/<city>/<city>_NNNNNN_000019_leftImg8bit.png (RGB) and, under gtFine/, the 16-bit `_gtFine_instanceIds.png` and the
    8-bit `_gtFine_labelIds.png`.  Image i has size sizes[i % len(sizes)] (height, width): stuff labels below 1000 in horizontal bands,
    and in the cells of a 3 x 6 grid 6-9 instances (connected, non-touching rectangles and ellipses, value label * 1000 + k, k from 0),
    two per label, and one "group" region stored as plain 26.  With n >= 4 every instance label 24..33 -- caravan 29 and
    trailer 30 included -- occurs in every split; the first two instances of image 0 have equal areas.  For tests and smoke runs of the
    data path only."""
    from PIL import Image
    r = np.random.default_rng(seed)
    stuff = (23, 11, 21, 7, 8)                                   # sky, building, vegetation, road, sidewalk
    for split in ("train", "val", "test"):
        for i in range(n):
            H, W = sizes[i % len(sizes)]
            city = cities[i % len(cities)]
            yy, xx = np.mgrid[0:H, 0:W]
            ids = np.zeros((H, W), np.uint16)
            for j, s in enumerate(stuff):
                ids[j * H // len(stuff):(j + 1) * H // len(stuff)] = s
            rgb = r.integers(0, 70, (H, W, 3)).astype(np.uint8)
            k = int(r.integers(6, 10))
            cells = [int(c) for c in r.permutation(18)[:k + 1]]
            if i == 0:
                cells = [0, 17] + [c for c in cells if c not in (0, 17)][:k - 1]
            ch, cw = H // 3, W // 6
            used = {}
            for j, cell in enumerate(cells):
                cy, cx = (cell // 6) * ch + ch / 2.0, (cell % 6) * cw + cw / 2.0
                a, b = r.uniform(0.36, 0.46) * ch, r.uniform(0.36, 0.46) * cw
                if i == 0 and j < 2:
                    a, b = 0.4 * ch, 0.4 * cw
                if (i == 0 and j < 2) or r.random() < 0.5:
                    m = (np.abs(yy - int(cy)) <= int(a)) & (np.abs(xx - int(cx)) <= int(b))
                else:
                    m = ((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2 <= 1.0
                if j == k:                                       # a group of cars: the label without an instance number
                    ids[m] = 26
                else:
                    label = INSTANCE_LABELS[(3 * i + j // 2) % 10]
                    ids[m] = label * 1000 + used.get(label, 0)
                    used[label] = used.get(label, 0) + 1
                rgb[m] = (r.integers(80, 255), r.integers(80, 255), r.integers(80, 255))
            stem = "%s_%06d_000019" % (city, i)
            for root in ("leftImg8bit", "gtFine"):
                os.makedirs(os.path.join(path, root, split, city), exist_ok=True)
            Image.fromarray(rgb).save(os.path.join(path, "leftImg8bit", split, city, stem + "_leftImg8bit.png"))
            Image.fromarray(ids).save(os.path.join(path, "gtFine", split, city, stem + "_gtFine_instanceIds.png"))
            lab = np.where(ids >= 1000, ids // 1000, ids).astype(np.uint8)
            Image.fromarray(lab).save(os.path.join(path, "gtFine", split, city, stem + "_gtFine_labelIds.png"))
    return path
