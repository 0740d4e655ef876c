"""Pascal VOC reader -- the reference's src/dataloader/pascal.py:17-79 on the base class of reader.py and the device loader of loader.py:
  host   : the split file, JPEG decode and the PIL bilinear `Scale` of the image, the nearest zoom of BOTH maps of ProcMasks/<name>.npy
           ([seg, ins], written by rsis_amd.pascal_precompute) to the image size; flip, the centred random crop and the decode cache are
           Reader's;
  device : normalisation, ONE affine warp shared by image, instance map and class map (`num_maps` = 2, used as they are), the targets
           (rsis_targets_from_maps).
Unlike leaves, the zoom range of the augmentation does not depend on --resize (pascal.py:47-51)."""
import os

import numpy as np

from .reader import Reader, scale_image, zoom_map

CLASSES = ["<eos>", "airplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "dining table", "dog", "horse",
           "motorcycle", "person", "potted plant", "sheep", "sofa", "train", "tv"]          # pascal.py:28-32
VOID_ID = 255


def voc_colormap(n=256):
    """the VOC colour map (VOCdevkit VOClabelcolormap): the bits of the index, three at a time, go to r, g, b from the top bit down"""
    cmap = np.zeros((n, 3), np.uint8)
    for i in range(n):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        cmap[i] = (r, g, b)
    return cmap


def palette_table():
    """(22, 4) uint8 rows (r, g, b, id): the 21 class colours and void (224, 224, 192) -> 255 -- the `palette` of the reference's
    dataset_utils.py; any other colour is id 0, so the object ids above 20 of SegmentationObject fall to 0 as they do there"""
    cmap = voc_colormap()
    ids = list(range(len(CLASSES))) + [VOID_ID]
    return np.array([tuple(cmap[i]) + (i,) for i in ids], np.uint8)


class PascalVOC(Reader):
    """reference PascalVOC(MyDataset): same constructor arguments, `classes`, `get_classes`, `get_sample_list`, `__len__`,
    `get_raw_sample`; `host_item` returns THREE arrays (image, instance map, class map)"""
    num_maps = 2

    def __init__(self, args, transform=None, target_transform=None, augment=False, split="train", resize=False, imsize=256):
        self._setup(args, transform, target_transform, augment, split, resize, imsize, crop=args.batch_size != 1,   # pascal.py:41-51
                    zoom_range=(args.zoom, max(args.zoom * 2, 1.0)))
        self.classes = list(CLASSES)
        self.num_classes = len(self.classes)
        self.image_dir = os.path.join(args.pascal_dir, "JPEGImages")
        self.masks_dir = os.path.join(args.pascal_dir, "ProcMasks")
        with open(os.path.join(args.pascal_dir, "ImageSets", "Segmentation", split + ".txt"), "r") as lines:   # :60-66
            self.image_files = [line.rstrip("\n") for line in lines]

    def image_path(self, index):
        return os.path.join(self.image_dir, self.image_files[index].rstrip() + ".jpg")

    def get_raw_sample(self, index):
        """(PIL RGB image, instance-id map, class map) in raw size -- pascal.py:68-79"""
        from PIL import Image
        img = Image.open(self.image_path(index)).convert("RGB")
        path = os.path.join(self.masks_dir, self.image_files[index].rstrip() + ".npy")
        if not os.path.exists(path):
            raise IOError("%s is missing: run `python -m rsis_amd.pascal_precompute --pascal_dir %s --split %s` first"
                          % (path, os.path.dirname(self.masks_dir), self.split))
        mask = np.load(path)
        return img, mask[:, :, 1], mask[:, :, 0]

    def _decode(self, index):
        img, ins, seg = self.get_raw_sample(index)
        im = scale_image(img, self.imsize, self.resize)
        return im, zoom_map(ins, im.shape[1:]), zoom_map(seg, im.shape[1:])      # dataset_utils.py:27-38,133-140: both maps


def synthesize_pascal_dir(path, n=6, sizes=((48, 64), (75, 50)), seed=0, classes=(2, 7, 15)):
    """Write a small VOC-shaped tree: JPEGImages/*.jpg, colour SegmentationClass / SegmentationObject PNGs whose instances carry the
    two-pixel void outline of the real annotations, ImageSets/Segmentation/{train,val}.txt (the last max(2, n // 3) images validate).
    Image i has size sizes[i % len(sizes)] (height, width) and 2-7 instances (rectangles and ellipses in the cells of a 3 x 3 grid) of
    the given classes, every class used somewhere; the first two instances of image 0 have equal areas.  ProcMasks and VOCGT_*.pkl
    are NOT written: that is rsis_amd.pascal_precompute.  For tests and smoke runs of the data path only."""
    from PIL import Image
    for sub in ("JPEGImages", "SegmentationClass", "SegmentationObject", os.path.join("ImageSets", "Segmentation")):
        os.makedirs(os.path.join(path, sub), exist_ok=True)
    r = np.random.default_rng(seed)
    cmap = voc_colormap()
    void = np.array((224, 224, 192), np.uint8)
    names = []
    for i in range(n):
        H, W = sizes[i % len(sizes)]
        yy, xx = np.mgrid[0:H, 0:W]
        k = int(r.integers(2, 8))
        cells = [int(c) for c in r.permutation(9)[:k]]
        if i == 0:
            cells[:2] = [0, 8]                                   # (two cells that do not touch)
            cells[2:] = [c for c in (4, 2, 6, 1, 3)][:k - 2]
        ins = np.zeros((H, W), np.uint8)
        seg = np.zeros((H, W), np.uint8)
        rgb = r.integers(0, 70, (H, W, 3)).astype(np.uint8)
        ch, cw = H // 3, W // 3
        for j, cell in enumerate(cells):
            cy, cx = (cell // 3) * ch + ch / 2.0, (cell % 3) * cw + cw / 2.0
            a, b = r.uniform(0.3, 0.45) * ch, r.uniform(0.3, 0.45) * cw
            if i == 0 and j < 2:
                a, b = 0.4 * ch, 0.4 * cw
            if (i == 0 and j < 2) or r.random() < 0.5:
                m = (np.abs(yy - int(cy)) <= int(a)) & (np.abs(xx - int(cx)) <= int(b))
            else:
                m = ((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2 <= 1.0
            cls = classes[(i + j) % len(classes)]
            ins[m], seg[m] = j + 1, cls
            rgb[m] = (r.integers(80, 255), r.integers(80, 255), r.integers(80, 255))
        edge = np.zeros((H, W), bool)                             # a pixel whose right / lower neighbour is another instance, and that one
        dv, dh = ins[1:, :] != ins[:-1, :], ins[:, 1:] != ins[:, :-1]
        edge[1:, :] |= dv
        edge[:-1, :] |= dv
        edge[:, 1:] |= dh
        edge[:, :-1] |= dh
        obj, cla = cmap[ins], cmap[seg]
        obj[edge], cla[edge] = void, void
        name = "2007_%06d" % i
        Image.fromarray(rgb).save(os.path.join(path, "JPEGImages", name + ".jpg"), quality=90)
        Image.fromarray(cla).save(os.path.join(path, "SegmentationClass", name + ".png"))
        Image.fromarray(obj).save(os.path.join(path, "SegmentationObject", name + ".png"))
        names.append(name)
    n_val = min(n - 1, max(2, n // 3))
    for split, part in (("train", names[:n - n_val]), ("val", names[n - n_val:])):
        with open(os.path.join(path, "ImageSets", "Segmentation", split + ".txt"), "w") as f:
            f.write("".join(s + "\n" for s in part))
    return path
