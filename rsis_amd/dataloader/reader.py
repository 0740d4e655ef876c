"""The base class of the dataset readers (leaves, pascal, cityscapes, coco) -- what the reference's MyDataset (src/dataloader/dataset.py:
47-84 + dataset_utils.py:27-57) does on the host, once: the common constructor state, the decode cache, the PIL `Scale` of the image,
the nearest zoom of a label map, the flip / crop draws and the generic `host_item`.  A reader adds its file list, `get_raw_sample` and
`_decode`.

The contract with DeviceLoader (loader.py): every reader answers the same questions, with these defaults --
  num_maps       how many int32 maps `host_item` returns after the image (1);
  same_size      whether un-cropped samples share one size, so that they can be batched (False);
  stage_batch    per batch, on the staging thread: host items -> (int64 table, layout) for ONE more host-to-device copy, or
                 (None, None) (the default);
  maps_to_warp   on the copy stream, before the warp: the copied maps (and table) -> the list of integer maps to warp (the maps);
  label_maps     on the copy stream, after the warp: the warped integer maps -> (instance map, class map) (the two maps as they are);
  ignore_map     on the copy stream, after the warp: the warped integer maps -> the (B, H, W) ignore region of the batch (non-zero / True =
                 the pixel is left out of the mask loss), or None (the default: no such region, the loader yields 5-tuples).  A reader
                 with a source for it answers only under `--ignore_regions`; the warp's zero fill outside the frame counts."""
import os
import sys

import numpy as np

from .augment import RandomAffine


def scale_image(img, S, resize):
    """transforms.Scale((S, S)) if `resize`, else transforms.Scale(S) (shorter side -> S), PIL bilinear -> (3, h, w) uint8"""
    from PIL import Image
    if resize:
        img = img.resize((S, S), Image.BILINEAR)
    else:
        w, h = img.size
        if w <= h:
            img = img.resize((S, max(S, int(S * h / w))), Image.BILINEAR)
        else:
            img = img.resize((max(S, int(S * w / h)), S), Image.BILINEAR)
    return np.ascontiguousarray(np.asarray(img, dtype=np.uint8).transpose(2, 0, 1))


def zoom_map(m, size):
    """nearest resize of a label map to `size` = (h, w): scipy zoom(order=0, mode='nearest'), dataset_utils.py:133-140"""
    from scipy.ndimage import zoom
    return np.ascontiguousarray(zoom(m, [float(size[0]) / m.shape[0], float(size[1]) / m.shape[1]], mode="nearest", order=0))


def flip_crop(a, flip, crop, S):
    """the flipped, cropped view of an (..., h, w) array"""
    if flip:
        a = a[..., ::-1]
    if crop is not None:
        a = a[..., crop[0]:crop[0] + S, crop[1]:crop[1] + S]
    return a


_WARNED = set()


def warn_once(msg):
    """one line on stderr, once per process"""
    if msg not in _WARNED:
        _WARNED.add(msg)
        print(msg, file=sys.stderr, flush=True)


class Reader(object):
    """reference MyDataset: `classes`, `get_classes`, `get_sample_list`, `__len__`, `get_raw_sample`; plus `image_path`, `raw_size`,
    `host_item` and the loader contract of the module docstring"""
    num_maps = 1
    same_size = False
    has_ignore_source = False       # the dataset marks regions "objects here, not outlined" (coco, cityscapes)

    def _setup(self, args, transform, target_transform, augment, split, resize, imsize, crop, zoom_range):
        """the constructor state every reader has; `crop` and `zoom_range` are what differs between the datasets"""
        self.split = split
        self.max_seq_len = args.gt_maxseqlen
        self.transform, self.target_transform = transform, target_transform
        self.batch_size = args.batch_size
        self.crop = crop
        self.flip = augment
        self.augment, self.resize, self.imsize, self.zoom = augment, resize, imsize, args.zoom
        self.augmentation_transform = None
        if augment:
            self.augmentation_transform = RandomAffine(rotation_range=args.rotation, translation_range=args.translation,
                                                       shear_range=args.shear, zoom_range=zoom_range, interp="nearest")
        self.ignore_regions = bool(getattr(args, "ignore_regions", False))
        if self.ignore_regions and not self.has_ignore_source:
            warn_once("--ignore_regions: %s has no source for an ignore region (no crowd / group records): no map is produced"
                      % type(self).__name__)
        self._cache, self._cache_bytes = {}, 0
        self._cache_limit = int(float(os.environ.get("RSIS_LOADER_CACHE_MB", "1024")) * (1 << 20))

    def get_classes(self):
        return self.classes

    def get_sample_list(self):
        return self.image_files

    def __len__(self):
        return len(self.image_files)

    def image_path(self, index):
        return self.image_files[index]

    def raw_size(self, index):
        """(height, width) of the original image, from the file's header"""
        from PIL import Image
        with Image.open(self.image_path(index)) as im:
            w, h = im.size
        return h, w

    def _decoded(self, index):
        """the deterministic part of host_item -- decode, the bilinear resize of the image, the nearest zoom of the maps -- kept after its
        first evaluation: the reference re-decodes every file in every epoch (dataset.py:47-54), which at CVPPP's 128 images is 7-15 ms
        of host time per image for the same bytes, and made `train.py` on this loader host-bound (NOTES (54): 62 images/s at batch 2).
        Bounded by RSIS_LOADER_CACHE_MB (default 1024; 0 = off): A1 at 256 x 256 is 58 MB.  The random part (flip, crop) works on views
        and copies, never on the cached arrays."""
        hit = self._cache.get(index)
        if hit is not None:
            return hit
        item = self._decode(index)
        nbytes = sum(a.nbytes for a in item)
        if self._cache_bytes + nbytes <= self._cache_limit:
            self._cache[index] = item
            self._cache_bytes += nbytes
        return item

    def _draw(self, size, rng):
        """the per-sample draws for a decoded image of `size` = (h, w) -> (flip, crop (oh, ow) or None): the flip of
        dataset_utils.py:51-55, then the centred random crop of transforms.py:15-21, width before height"""
        flip = bool(self.flip and rng.random() < 0.5)
        if not self.crop:
            return flip, None
        rw, rh = (size[1] - self.imsize) // 2, (size[0] - self.imsize) // 2
        ow = 0 if rw <= 0 else rng.randrange(rw)
        oh = 0 if rh <= 0 else rng.randrange(rh)
        return flip, (oh, ow)

    def host_item(self, index, rng):
        """everything of dataset.py:47-62 that is decoding / index arithmetic -> (uint8 image (3, S, S), `num_maps` int32 maps (S, S));
        un-cropped sizes when `crop` is off"""
        im, *maps = self._decoded(index)
        flip, crop = self._draw(im.shape[1:], rng)
        return (np.ascontiguousarray(flip_crop(im, flip, crop, self.imsize)),) + tuple(
            np.ascontiguousarray(flip_crop(m, flip, crop, self.imsize).astype(np.int32)) for m in maps)

    def stage_batch(self, items, S):
        return None, None

    def maps_to_warp(self, maps, table, layout):
        return maps

    def label_maps(self, maps):
        ins, seg = maps
        return ins, seg

    def ignore_map(self, maps):
        return None
