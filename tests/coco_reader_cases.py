"""Shared by the COCO reader tests: the expected values, written by hand in numpy.

masks      : tests/polymask_golden.record_mask (pinned bit for bit to the reference's mask API by tests/golden/polymask.npz) for
             polygons, polymask_golden.decode for uncompressed counts.
paint_rule : the rule of rsis_paint_instance_maps (include/rsis_hip.h): per pixel the covering record of the smallest mask area wins,
             equal areas go to the lower index, a mask of area 0 never wins; sampled through two index tables, 0 outside the image.
host_maps  : what the other readers do on the host -- compose at native size, scipy zoom(order=0, mode='nearest') of both maps, flip,
             crop -- for a sample of the COCO reader.
Nothing here calls the code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polymask_golden as PG  # noqa: E402


def words_of(length):
    return 2 * ((int(length) + 127) // 128)


def pack(mask_cm):
    """(h * w,) 0/1 in column-major element order -> (words_of,) int64 row: element e is bit e % 64 of word e / 64"""
    n = len(mask_cm)
    b = np.zeros((64 * words_of(n),), np.uint8)
    b[:n] = mask_cm
    return np.packbits(b, bitorder="little").view(np.uint64).view(np.int64)


def compose(masks_cm, sizes, inst_ids, class_ids, hw):
    """native (ins, seg) int32 (h, w) of one sample whose records all have the native size hw: winner by (area, index)"""
    h, w = hw
    ins, seg = np.zeros((h, w), np.int32), np.zeros((h, w), np.int32)
    best = np.full((h, w), 2 ** 62, np.int64)
    for m, s, i, c in zip(masks_cm, sizes, inst_ids, class_ids):
        assert tuple(s) == (h, w)
        m2 = m.reshape(w, h).T > 0
        a = int(m2.sum())
        if a == 0:
            continue
        take = m2 & (a < best)
        ins[take], seg[take], best[take] = i, c, a
    return ins, seg


def paint_rule(masks_cm, sizes, inst_ids, class_ids, src_y, src_x):
    """one sample by the kernel's rule, records of ANY native sizes: (ins, seg) int32 (len(src_y), len(src_x))"""
    Ho, Wo = len(src_y), len(src_x)
    ins, seg = np.zeros((Ho, Wo), np.int32), np.zeros((Ho, Wo), np.int32)
    best = np.full((Ho, Wo), 2 ** 62, np.int64)
    sy, sx = np.asarray(src_y, np.int64)[:, None], np.asarray(src_x, np.int64)[None, :]
    for m, (h, w), i, c in zip(masks_cm, sizes, inst_ids, class_ids):
        a = int(np.asarray(m).sum())
        if a == 0:
            continue
        inside = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
        m2 = m.reshape(w, h).T
        hit = inside & (m2[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)] > 0)
        take = hit & (a < best)
        ins[take], seg[take], best[take] = i, c, a
    return ins, seg


def zoom_nearest(a, size):
    """the readers' resize of a label map: scipy zoom(order=0, mode='nearest') to (h, w)"""
    from scipy.ndimage import zoom
    return zoom(a, [float(size[0]) / a.shape[0], float(size[1]) / a.shape[1]], mode="nearest", order=0)


def ramp_tables(native, resized):
    """(src_y, src_x) as scipy sees them: zoom of an index ramp along each axis"""
    ys = np.repeat(np.arange(native[0], dtype=np.int64)[:, None], native[1], axis=1)
    xs = np.repeat(np.arange(native[1], dtype=np.int64)[None, :], native[0], axis=0)
    zy, zx = zoom_nearest(ys, resized), zoom_nearest(xs, resized)
    assert zy.shape == tuple(resized) and (zy == zy[:, :1]).all() and (zx == zx[:1, :]).all()
    return zy[:, 0].astype(np.int32), zx[0, :].astype(np.int32)


def file_sample(annotation, image_id):
    """(records of the image that the reader paints, native (h, w)) from a parsed COCO file: non-crowd polygon records in file order;
    each (parts, class index) with class index = 1 + rank of the category id"""
    cats = sorted(c["id"] for c in annotation["categories"])
    im = [i for i in annotation["images"] if i["id"] == image_id][0]
    recs = [(a["segmentation"], 1 + cats.index(a["category_id"])) for a in annotation["annotations"]
            if a["image_id"] == image_id and not a.get("iscrowd", 0) and isinstance(a["segmentation"], list)]
    return recs, (im["height"], im["width"])


def host_maps(annotation, image_id, resized, flip=False, crop=None, S=None):
    """(ins, seg) of one sample as the host pipeline of the other readers makes them"""
    recs, (h, w) = file_sample(annotation, image_id)
    masks = [PG.record_mask([np.asarray(p, np.float64) for p in parts], h, w) for parts, _c in recs]
    ins, seg = compose(masks, [(h, w)] * len(recs), range(1, len(recs) + 1), [c for _p, c in recs], (h, w))
    ins, seg = zoom_nearest(ins, resized), zoom_nearest(seg, resized)
    if flip:
        ins, seg = ins[:, ::-1], seg[:, ::-1]
    if crop is not None:
        ins, seg = ins[crop[0]:crop[0] + S, crop[1]:crop[1] + S], seg[crop[0]:crop[0] + S, crop[1]:crop[1] + S]
    return np.ascontiguousarray(ins), np.ascontiguousarray(seg)


def eval_samples():
    """the `eval` set of tests/golden/polymask.npz as painter samples: per image (masks, sizes, instance ids, class ids, (h, w)) of its
    polygon records (the crowd record, uncompressed counts, is decoded and painted too: the kernel takes rows of either origin)"""
    E = PG.load()["eval"]
    out = []
    for im in E["images"]:
        h, w = im["height"], im["width"]
        masks, cls = [], []
        for r in E["gt_poly"]:
            if r["image_id"] != im["id"]:
                continue
            seg = r["segmentation"]
            if isinstance(seg, dict):
                masks.append(PG.decode(seg["counts"], h * w))
            else:
                masks.append(PG.record_mask([np.asarray(p, np.float64) for p in seg], h, w))
            cls.append(int(r["category_id"]) + 10)
        out.append((masks, [(h, w)] * len(masks), list(range(1, len(masks) + 1)), cls, (h, w)))
    return out
