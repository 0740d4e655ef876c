"""Numpy statements of the two rules that make an ignore map (--ignore_regions), for test_gpu_ignore_loader.py and, on
hand-written arrays, test_ignore_host.py.  Host only; nothing here touches the device.

  Cityscapes : ignore = raw < 1000 and CLASS_OF_LABEL[raw] > 0 on the WARPED raw `instanceIds` values -- the group regions of trained
               classes; void labels, groups of untrained labels and the warp's zero fill stay counted.
  COCO       : decode the image's crowd records at native size, OR them, resample through the index tables (nearest resize, flip,
               crop), clear where an instance was painted."""
import numpy as np

import coco_reader_cases as CR


def cityscapes_ignore(raw, class_of_label):
    raw = np.asarray(raw, np.int64)
    table = np.asarray(class_of_label, np.int64)
    cls = np.where((raw >= 0) & (raw < len(table)), table[np.clip(raw, 0, len(table) - 1)], 0)
    return (raw < 1000) & (cls > 0)


def crowd_mask(seg, h, w):
    """(h, w) bool of one crowd record: uncompressed run counts (column-major runs, zeros first) or polygon parts"""
    if isinstance(seg, dict):
        flat = CR.PG.decode(seg["counts"], h * w)
    else:
        flat = CR.PG.record_mask([np.asarray(p, np.float64) for p in seg], h, w)
    return np.asarray(flat).reshape(w, h).T > 0


def coco_ignore(annotation, image_id, src_y, src_x, ins):
    """(Ho, Wo) uint8: the OR of the image's crowd records at (src_y, src_x), cleared where `ins` (the painted instance map at the output
    size) holds an instance"""
    im = [i for i in annotation["images"] if i["id"] == image_id][0]
    h, w = im["height"], im["width"]
    m = np.zeros((h, w), bool)
    for a in annotation["annotations"]:
        if a["image_id"] == image_id and a.get("iscrowd", 0):
            m |= crowd_mask(a["segmentation"], h, w)
    out = m[np.asarray(src_y, np.int64)][:, np.asarray(src_x, np.int64)]
    return (out & (np.asarray(ins) == 0)).astype(np.uint8)
