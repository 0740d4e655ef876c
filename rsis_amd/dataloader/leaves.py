"""CVPPP A1 leaves reader -- the reference's src/dataloader/leaves.py:9-113 on the base class of reader.py (which holds what
dataset.py:47-84 + dataset_utils.py:28-58 do on the host) and the device loader of loader.py (BASELINE
configs[0]).  Its own: the file list and train / val split (leaves.py:64-94), `get_raw_sample`, and the class map derived on the device
as `ins > 0` (leaves.py:105-106).
Deviation: the file list is sorted (the reference takes glob's order, which is file-system dependent)."""
import glob
import os

import numpy as np

from .reader import Reader, scale_image, zoom_map


class LeavesDataset(Reader):
    """reference LeavesDataset(MyDataset): same constructor arguments, `classes`, `get_raw_sample`, `__len__`, `get_sample_list`;
    `host_item` returns (image, instance map)"""

    def __init__(self, args, transform=None, target_transform=None, augment=False, split="train", resize=False, imsize=256):
        self._setup(args, transform, target_transform, augment, split, resize, imsize, crop=args.batch_size != 1,   # leaves.py:31-47
                    zoom_range=(args.zoom, 1) if resize else None)
        self.classes = ["<eos>", "leaf"]                                   # leaves.py:20
        self.num_classes = len(self.classes)
        total = sorted(glob.glob(os.path.join(args.leaves_dir, "*_rgb.png")))
        gts = [w.replace("_rgb", "_label") for w in total]
        if split == "train":                                                # :72-94: the first 96 images train, the rest validate
            self.image_files, self.gt_files = total[:96], gts[:96]
        elif split == "val":
            self.image_files, self.gt_files = total[96:], gts[96:]
        else:
            self.image_files = sorted(glob.glob(os.path.join(args.leaves_test_dir, "*_rgb.png")))
            self.gt_files = []

    def get_raw_sample(self, index):
        """(PIL RGB image, instance-id map, class map) in raw size -- leaves.py:96-113"""
        from PIL import Image
        img = Image.open(self.image_files[index]).convert("RGB")
        if self.split != "test":
            gt = np.array(Image.open(self.gt_files[index]))
            ins = gt.copy()
            seg = gt.copy()
            seg[seg > 0] = 1
            return img, ins, seg
        fake = np.array(img)[:, :, 0]
        return img, fake, fake

    def _decode(self, index):
        img, ins, _seg = self.get_raw_sample(index)
        im = scale_image(img, self.imsize, self.resize)
        return im, zoom_map(ins, im.shape[1:])

    def label_maps(self, maps):
        ins, = maps
        return ins, (ins > 0).long()                                        # leaves.py:105-106


def synthesize_leaves_dir(path, n=100, size=(192, 208), seed=0):
    """Write n synthetic CVPPP-A1-style pairs plantNNN_rgb.png / plantNNN_label.png (instance ids 1..k, 0 = background): elliptical
    'leaves' on a textured background.  For tests and smoke runs of the data path only."""
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    r = np.random.default_rng(seed)
    H, W = size
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        rgb = r.integers(0, 80, (H, W, 3)).astype(np.uint8)
        lab = np.zeros((H, W), np.uint8)
        for k in range(1, int(r.integers(3, 9)) + 1):
            cy, cx = r.uniform(0.2, 0.8) * H, r.uniform(0.2, 0.8) * W
            a, b, th = r.uniform(8, 0.25 * H), r.uniform(6, 0.15 * W), r.uniform(0, np.pi)
            u = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th)
            v = -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
            m = (u / a) ** 2 + (v / b) ** 2 <= 1.0
            lab[m] = k
            rgb[m] = (r.integers(20, 90), r.integers(120, 255), r.integers(20, 90))
        Image.fromarray(rgb).save(os.path.join(path, "plant%03d_rgb.png" % i))
        Image.fromarray(lab).save(os.path.join(path, "plant%03d_label.png" % i))
    return path
