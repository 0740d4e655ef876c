"""Offline preparation of Pascal VOC -- counterpart of reference src/dataloader/pascal_precompute.py:36-101:

    python -m rsis_amd.pascal_precompute --pascal_dir D --split S [--forcegen]

For every image of ImageSets/Segmentation/<S>.txt: SegmentationClass/<name>.png and SegmentationObject/<name>.png are read as RGB and
mapped to ids by colour (the 21 VOC colours and void (224, 224, 192) -> 255, anything else -> 0: rsis_palette_to_ids, where the
reference does a Python dict lookup per pixel), void pixels of the class map become the ignore mask and are cleared in both maps,
and uint8 (h, w, 2) = [seg, ins] goes to ProcMasks/<name>.npy -- what dataloader/pascal.py reads.  <D>/VOCGT_<S>.pkl gets the COCO-style
ground truth rsis_amd.eval scores against: per image one record per instance id in ascending order (category = the smallest class
under the instance), then 20 `ignore = 1` records that carry the ignore mask, one per category 1..20; the run-length encodings of
all instances of an image come from ONE launch over the id map (rsis_idmap_rle_encode), the text from rsis_rle_to_string.

Kept from the reference: object ids above 20 have colours outside the table and fall to 0 (background); the 20 ignore records are
written for EVERY image (its `len(np.unique(ignore_mask)) == 0` test is never true).  Deviation: when ProcMasks/<name>.npy already
exists (no --forcegen) the reference reuses the ignore mask of the PREVIOUS image (or fails on the first); here the ignore mask is
recomputed from the class PNG."""
import argparse
import ctypes
import os
import pickle

import numpy as np
import torch

from ._lib import check, lib, ptr, stream
from .dataloader.pascal import CLASSES, VOID_ID, palette_table


def ids_from_colors_numpy(rgb, table=None):
    """numpy statement of the colour lookup: rgb (h, w, 3) uint8 -> (h, w) uint8 ids (first matching table row wins, no match = 0)"""
    table = palette_table() if table is None else np.asarray(table, np.uint8)
    rgb = np.asarray(rgb, np.uint8)
    key = rgb[..., 0].astype(np.int64) | (rgb[..., 1].astype(np.int64) << 8) | (rgb[..., 2].astype(np.int64) << 16)
    out = np.zeros(key.shape, np.uint8)
    for r, g, b, i in table[::-1]:
        out[key == (int(r) | (int(g) << 8) | (int(b) << 16))] = i
    return out


def precompute_numpy(cls_rgb, obj_rgb):
    """pascal_precompute.py:36-59 in numpy: -> (masks (h, w, 2) uint8 = [seg, ins], ignore (h, w) uint8)"""
    seg, ins = ids_from_colors_numpy(cls_rgb), ids_from_colors_numpy(obj_rgb)
    ignore = seg == VOID_ID
    ins[ignore] = 0
    seg[ignore] = 0
    return np.stack([seg, ins], axis=-1), ignore.astype(np.uint8)


def palette_to_ids(rgb, table):
    """rgb: (..., 3) CUDA uint8, table: (n <= 256, 4) CUDA uint8 rows (r, g, b, id) -> (...) CUDA uint8 ids (rsis_palette_to_ids)"""
    if not (rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.shape[-1] == 3 and table.is_cuda and table.dtype == torch.uint8):
        raise ValueError("palette_to_ids: CUDA uint8 tensors (..., 3) and (n, 4) are required (there is no CPU path)")
    rgb, table = rgb.contiguous(), table.contiguous()
    out = torch.empty(rgb.shape[:-1], dtype=torch.uint8, device=rgb.device)
    if out.numel():
        check(lib().rsis_palette_to_ids(ptr(rgb), out.numel(), ptr(table), int(table.shape[0]), ptr(out), stream()), "rsis_palette_to_ids")
    return out


def idmap_rle_counts(idmap, ids, cap=None):
    """idmap: (h, w) CUDA uint8, ids: k integers -> k uint32 arrays: the run counts of (idmap == id) in pycocotools' column-major order,
    from one launch of rsis_idmap_rle_encode (a second one when a mask has more than `cap` runs)"""
    if not (idmap.is_cuda and idmap.dtype == torch.uint8 and idmap.dim() == 2):
        raise ValueError("idmap_rle_counts: idmap must be a (h, w) CUDA uint8 tensor")
    ids = [int(v) for v in ids]
    if not ids:
        return []
    idmap = idmap.contiguous()
    h, w = idmap.shape
    k = len(ids)
    ids_d = torch.tensor(ids, dtype=torch.int32, device=idmap.device)
    cap = min(h * w + 1, 1 << 12) if cap is None else int(cap)
    while True:
        counts = torch.empty((k, cap), dtype=torch.int32, device=idmap.device)
        nruns = torch.empty((k,), dtype=torch.int32, device=idmap.device)
        check(lib().rsis_idmap_rle_encode(ptr(idmap), h, w, ptr(ids_d), k, ptr(counts), cap, ptr(nruns), stream()), "rsis_idmap_rle_encode")
        nr = nruns.cpu().numpy()
        if (nr > 0).all():
            break
        cap = int(-nr.min())                                      # a mask with more runs than expected: retry with room for all
    host = counts[:, :int(nr.max())].cpu().numpy().view(np.uint32)
    return [np.ascontiguousarray(host[j, :nr[j]]) for j in range(k)]


def rle_strings(counts_list):
    """uint32 run counts -> pycocotools' compressed text (bytes), rsis_rle_to_string"""
    L = lib()
    out = []
    for c in counts_list:
        buf = ctypes.create_string_buffer(7 * len(c) + 8)
        ln = L.rsis_rle_to_string(c.ctypes.data_as(ctypes.c_void_p), len(c), buf, len(buf))
        if ln < 0:
            raise RuntimeError("rsis_rle_to_string: buffer too small")
        out.append(buf.raw[:ln])
    return out


def device_encoder(device="cuda"):
    """encode(idmap (h, w) uint8 numpy, ids) -> list of compressed RLE texts, on the device"""
    def encode(idmap, ids):
        d = torch.from_numpy(np.ascontiguousarray(idmap, dtype=np.uint8)).to(device)
        return rle_strings(idmap_rle_counts(d, ids))
    return encode


def create_annotation(imname, counts_text, size, class_id, score, crowd):
    """pascal_precompute.py:18-34, with the encoded mask given"""
    class_id = int(class_id)
    return {"image_id": imname.rstrip(), "category_id": class_id, "category_name": CLASSES[class_id],
            "segmentation": {"size": [int(size[0]), int(size[1])], "counts": counts_text}, "score": score, "ignore": crowd}


def make_records(name, masks, ignore, encode):
    """pascal_precompute.py:70-101 make_coco: the instance records in ascending id order (np.unique(ins)[1:]: the smallest id present
    is the background), then the 20 ignore records.  encode(idmap, ids) -> RLE texts of (idmap == id)."""
    seg, ins = masks[:, :, 0], masks[:, :, 1]
    size = ins.shape
    ids = [int(v) for v in np.unique(ins)[1:]]
    anns = []
    for i, text in zip(ids, encode(ins, ids)):
        anns.append(create_annotation(name, text, size, np.unique(seg[ins == i])[0], 1, 0))
    ign_text = encode(np.asarray(ignore, np.uint8), [1])[0]
    for c in range(1, len(CLASSES)):
        anns.append(create_annotation(name, ign_text, size, c, 1, 1))
    return anns


def get_imnames(pascal_dir, split):
    with open(os.path.join(pascal_dir, "ImageSets", "Segmentation", split + ".txt"), "r") as lines:
        return [line.rstrip() for line in lines]


def _read_rgb(path, device):
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8).copy()).to(device)


def precompute(name, pascal_dir, table, want_masks=True):
    """both PNGs of one image through rsis_palette_to_ids -> (masks (h, w, 2) uint8 numpy or None, ignore (h, w) uint8 numpy)"""
    dev = table.device
    seg = palette_to_ids(_read_rgb(os.path.join(pascal_dir, "SegmentationClass", name + ".png"), dev), table)
    ignore = seg == VOID_ID
    if not want_masks:
        return None, ignore.to(torch.uint8).cpu().numpy()
    ins = palette_to_ids(_read_rgb(os.path.join(pascal_dir, "SegmentationObject", name + ".png"), dev), table)
    ins = ins.masked_fill(ignore, 0)
    seg = seg.masked_fill(ignore, 0)
    return torch.stack([seg, ins], dim=-1).cpu().numpy(), ignore.to(torch.uint8).cpu().numpy()


def run(pascal_dir, split, forcegen=False, device="cuda", verbose=True):
    save_dir = os.path.join(pascal_dir, "ProcMasks")
    os.makedirs(save_dir, exist_ok=True)
    table = torch.from_numpy(palette_table()).to(device)
    encode = device_encoder(device)
    anns = []
    for name in get_imnames(pascal_dir, split):
        path = os.path.join(save_dir, name + ".npy")
        if forcegen or not os.path.isfile(path):
            masks, ignore = precompute(name, pascal_dir, table)
            np.save(path, masks)
        else:
            if verbose:
                print("Found masks for sample %s. Skipping." % name)
            masks = np.load(path)
            _, ignore = precompute(name, pascal_dir, table, want_masks=False)
        anns.extend(make_records(name, masks, ignore, encode))
    out = os.path.join(pascal_dir, "VOCGT_%s.pkl" % split)
    with open(out, "wb") as f:
        pickle.dump(anns, f, protocol=2)
    if verbose:
        print("%d ground-truth records -> %s" % (len(anns), out))
    return anns


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pascal_dir", required=True)
    ap.add_argument("--split", default="train")
    ap.add_argument("--forcegen", dest="forcegen", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rsis_amd.pascal_precompute needs the GPU: the HIP library is the only compute path")
    run(a.pascal_dir, a.split, a.forcegen)


if __name__ == "__main__":
    main()
