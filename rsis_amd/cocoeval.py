"""COCO 'segm' evaluation on the device -- counterpart of the second half of reference src/eval.py (eval.py:365-398) and of the
(modified) pycocotools COCOeval it calls (src/coco/PythonAPI/pycocotools/cocoeval.py), for iouType = 'segm' with masks as compressed
RLE, as the polygons / uncompressed RLE of a standard COCO annotation file, or as device tensors.  pycocotools itself is not used.

    python -m rsis_amd.cocoeval --gt GT.json --dt PRED.json [-max_dets N] [--ignore_cats] [--all_classes] [--all_images]

Where the work runs (rsis_amd/csrc/maskeval.hip, polymask.hip): masks become 64-bit words on the device (rsis_mask_pack_bits from the
uint8 output of rsis_mask_resize_threshold, rsis_rle_to_bits from run counts, rsis_poly_to_bits from polygons: the rasterisation of
maskApi.c rleFrPoly + rleMerge, bit for bit); ONE grouped launch counts the intersections of every (detection
mask, ground-truth mask) pair of every image (rsis_mask_intersect_batch) -- once per pair of distinct masks, however many records
(categories) share a mask; one launch forms the float64 IoU matrices of all (image, category) cells, one runs the greedy matching
of all (image, category, area range) cells.  The host sorts (numpy, stable, vectorised over all records), and accumulates the few
thousand precision / recall numbers in float64 in the reference's order of operations, so that they agree with it exactly.

Differences from the reference that are kept on purpose: its 13 `stats` (cocoeval.py:453-467), the ignore flag read
from gt['ignore'] and the crowd rule from gt['iscrowd'] (independent inputs), `maxDets` indexed by position and selected by equality
(a duplicate such as [1, 100, 100] is averaged over both columns), evaluateImg run at the largest maxDets only.
"""
import argparse
import ctypes
import json
import sys

import numpy as np
import torch

from ._lib import check, lib, ptr, stream


def rle_from_string(s):
    """COCO compressed RLE text (str or bytes) -> uint32 run counts (starting with the run of zeros)"""
    if isinstance(s, str):
        s = s.encode("ascii")
    L = lib()
    out = np.empty((max(1, len(s)),), np.uint32)                   # every count takes at least one character
    m = L.rsis_rle_from_string(s, out.ctypes.data_as(ctypes.c_void_p), len(out))
    if m < 0:
        raise RuntimeError("rsis_rle_from_string: buffer too small")
    return out[:m].copy()


def rle_to_string(counts):
    """uint32 run counts -> COCO compressed RLE text (bytes)"""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.uint32))
    buf = ctypes.create_string_buffer(7 * len(c) + 8)
    ln = lib().rsis_rle_to_string(c.ctypes.data_as(ctypes.c_void_p), len(c), buf, len(buf))
    if ln < 0:
        raise RuntimeError("rsis_rle_to_string: buffer too small")
    return buf.raw[:ln]


def words_of(length):
    """row stride, in 64-bit words, of a bit-packed mask of `length` elements (even: rows are made of 16-byte cells)"""
    return 2 * ((int(length) + 127) // 128)


def pack_bits(masks):
    """masks: (n, len) CUDA uint8 (zero / non-zero) -> (bits (n, words_of(len)) int64, area (n,) int32), on the device"""
    if not masks.is_cuda or masks.dtype != torch.uint8 or masks.dim() != 2:
        raise ValueError("pack_bits: masks must be a (n, len) CUDA uint8 tensor")
    masks = masks.contiguous()
    n, ln = masks.shape
    bits = torch.empty((n, words_of(ln)), dtype=torch.int64, device=masks.device)
    area = torch.empty((n,), dtype=torch.int32, device=masks.device)
    if n:
        check(lib().rsis_mask_pack_bits(ptr(masks), n, ln, ptr(bits), bits.shape[1], ptr(area), stream()), "rsis_mask_pack_bits")
    return bits, area


def rle_to_bits(counts_list, lengths, device="cuda"):
    """counts_list: n uint32 count arrays, lengths: their masks' element counts -> (list of n (words,) int64 device rows, area (n,)
    int32 device tensor); all rows live in one buffer and are produced by one launch"""
    n = len(counts_list)
    for c, ln in zip(counts_list, lengths):
        if int(np.sum(c, dtype=np.int64)) != int(ln):
            raise ValueError("RLE counts sum to %d, the mask has %d elements" % (int(np.sum(c, dtype=np.int64)), int(ln)))
    if n == 0:
        return [], torch.empty((0,), dtype=torch.int32, device=device)
    m = np.array([len(c) for c in counts_list], np.int64)
    w = np.array([words_of(ln) for ln in lengths], np.int64)
    coff, boff = np.concatenate([[0], np.cumsum(m)]), np.concatenate([[0], np.cumsum(w)])
    desc = np.stack([coff[:-1], m, boff[:-1], w], axis=1).astype(np.int64)
    allc = np.concatenate(list(counts_list) + [np.zeros((1,), np.uint32)]).astype(np.uint32)    # (never empty)
    cd = torch.from_numpy(allc.view(np.int32)).to(device)
    dd = torch.from_numpy(desc).to(device)
    ends = torch.empty_like(cd)
    bits = torch.empty((int(boff[-1]),), dtype=torch.int64, device=device)
    area = torch.empty((n,), dtype=torch.int32, device=device)
    check(lib().rsis_rle_to_bits(ptr(cd), cd.numel(), ptr(dd), n, ptr(ends), ptr(bits), bits.numel(), ptr(area), stream()), "rsis_rle_to_bits")
    return [bits[int(boff[k]):int(boff[k + 1])] for k in range(n)], area


def segmentation_kind(seg):
    """The form of a COCO `segmentation`: 'rle' ({'size', 'counts': compressed text}), 'counts' ({'size', 'counts': list of run
    lengths}: uncompressed RLE, how an annotation file stores crowd regions) or 'polygons' (a list of parts, each a flat list
    [x0, y0, x1, y1, ...] of at least 3 points).  Anything else -- a bare box, a part with an odd count or fewer than 3 points, a
    coordinate that is not finite or too large for the 5x integer grid of the rasteriser -- raises ValueError."""
    if isinstance(seg, dict):
        if "counts" not in seg or "size" not in seg or len(seg["size"]) != 2:
            raise ValueError("an RLE segmentation needs 'size': [h, w] and 'counts'")
        c = seg["counts"]
        if isinstance(c, (list, tuple)):
            return "counts"
        if isinstance(c, (str, bytes)):
            return "rle"
        raise ValueError("RLE 'counts' must be compressed text or a list of run lengths, not %s" % type(c).__name__)
    if not isinstance(seg, (list, tuple)) or len(seg) == 0:
        raise ValueError("a segmentation is an RLE dict or a non-empty list of polygon parts")
    for part in seg:
        if not isinstance(part, (list, tuple, np.ndarray)):
            raise ValueError("a polygon segmentation is a list of parts, each a list [x0, y0, x1, y1, ...] (a bare box is not a mask)")
        if len(part) < 6 or len(part) % 2:
            raise ValueError("a polygon part needs at least 3 points and an even number of coordinates, not %d numbers" % len(part))
        try:
            v = np.asarray(part, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("polygon coordinates must be numbers")
        if v.ndim != 1 or not np.isfinite(v).all() or (np.abs(5.0 * v) >= 2.0 ** 30).any():
            raise ValueError("polygon coordinates must be finite with |5 * coordinate| < 2^30")
    return "polygons"


def poly_to_bits(parts_per_record, sizes, device="cuda"):
    """parts_per_record: n records, each a list of polygon parts [x0, y0, x1, y1, ...]; sizes: their images' (h, w) -> (list of n
    (words,) int64 device rows, area (n,) int32 device tensor), the form rle_to_bits returns.  A record's mask is the union of its
    parts, each rasterised as the COCO mask API does (rsis_amd/csrc/polymask.hip); one launch for all records of the call."""
    n = len(parts_per_record)
    if len(sizes) != n:
        raise ValueError("poly_to_bits: one (h, w) per record")
    if n == 0:
        return [], torch.empty((0,), dtype=torch.int32, device=device)
    xy, ptab, rtab, nv, npart, boff = [], [], [], 0, 0, 0
    for parts, (h, w) in zip(parts_per_record, sizes):
        if segmentation_kind(parts) != "polygons":
            raise ValueError("poly_to_bits: every record must be a list of polygon parts")
        h, w = int(h), int(w)
        if h < 1 or w < 1 or h * w >= 2 ** 31:
            raise ValueError("poly_to_bits: image size %d x %d" % (h, w))
        for part in parts:
            v = np.asarray(part, dtype=np.float64)
            xy.append(v)
            ptab.append((nv, len(v) // 2))
            nv += len(v) // 2
        rtab.append((npart, len(parts), h, w, boff, words_of(h * w), 0, 0))
        npart += len(parts)
        boff += words_of(h * w)
    xd = torch.from_numpy(np.concatenate(xy)).to(device)
    pd = torch.from_numpy(np.array(ptab, np.int64)).to(device)
    rd = torch.from_numpy(np.array(rtab, np.int64)).to(device)
    scratch = torch.empty((boff,), dtype=torch.int64, device=device)
    bits = torch.empty((boff,), dtype=torch.int64, device=device)
    area = torch.empty((n,), dtype=torch.int32, device=device)
    check(lib().rsis_poly_to_bits(ptr(xd), nv, ptr(pd), npart, ptr(rd), n, ptr(scratch), ptr(bits), boff, ptr(area), stream()),
          "rsis_poly_to_bits")
    return [bits[r[4]:r[4] + r[5]] for r in rtab], area


def _image_sizes(images):
    """`images` of COCOEvalDevice / add_gt: a list of COCO image dicts (id, height, width) or {image id: (h, w)} -> {id: (h, w)}"""
    if not images:
        return {}
    if isinstance(images, dict):
        return {k: (int(v[0]), int(v[1])) for k, v in images.items()}
    return {im["id"]: (int(im["height"]), int(im["width"])) for im in images}


class Params(object):
    """cocoeval.py:494-529 for iouType 'segm'"""

    def __init__(self):
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.iouType = 'segm'


class _Side(object):
    """the masks (device, bit-packed, per image) and the records of the ground truth or of the detections"""

    def __init__(self):
        self.chunks = {}       # image id -> list of (bits (U, words) int64, area (U,) int32)
        self.rows = {}         # image id -> number of mask rows so far
        self.length = {}       # image id -> elements per mask
        self.rec = []          # (image id, category, row, score, area or None, iscrowd, ignore, id)

    def add_chunk(self, image_id, bits, area, length):
        base = self.rows.get(image_id, 0)
        self.chunks.setdefault(image_id, []).append((bits, area))
        self.rows[image_id] = base + bits.shape[0]
        self.length[image_id] = int(length)
        return base


class COCOEvalDevice(object):
    """Drop-in for the reference's COCOeval(cocoGt, cocoDt, 'segm'): set `params`, then evaluate() / accumulate() / summarize().
    gt / dt: lists of COCO annotation records (image_id, category_id, segmentation = {'size': [h, w], 'counts': compressed RLE or a
    list of run lengths} or a list of polygons, score for detections; for ground truth `area` (default: the mask's), `iscrowd`,
    `ignore` (default 0), `id` (default: position + 1)); more can be added with add_gt / add_dt, or from device tensors with
    add_gt_masks / add_dt_masks.  A polygon record takes its image's size from `images` (COCO image dicts, or {image id: (h, w)}) or
    from an RLE record of the same image."""

    def __init__(self, gt=None, dt=None, device="cuda", images=None):
        self.params = Params()
        self.device = device
        self._gt, self._dt = _Side(), _Side()
        self._size = _image_sizes(images)                            # image id -> (h, w), from `images` and from RLE records
        self.eval, self.stats, self._res = {}, [], None
        self.keep_intersect_inputs = False                           # tools/bench_cocoeval.py: replay the grouped launch on its own
        if gt:
            self.add_gt(gt)
        if dt:
            self.add_dt(dt)
        if gt:
            self.params.imgIds = sorted(set(r["image_id"] for r in gt))
            self.params.catIds = sorted(set(r["category_id"] for r in gt))

    # ------------------------------------------------------------------ input ------------------------------------------------------------------
    def _add_records(self, side, records, is_gt, images=None):
        """records of any segmentation_kind.  Rows of an image, in order of first appearance: one per distinct compressed text
        (records that share a mask share its row), one per uncompressed-RLE or polygon record."""
        seen = {}                                                    # sizes this call states (kept at the end: a refused call changes nothing)
        known = self._size

        def note(img, hw):
            if seen.setdefault(img, known.get(img, hw)) != hw:
                raise ValueError("image %r has masks of different sizes" % (img,))
        for img, hw in _image_sizes(images).items():
            note(img, hw)
        per_img = {}                                                 # image id -> (list of rows: (kind, payload), {counts text: row})
        todo = []
        for r in records:
            seg = r["segmentation"]
            kind = segmentation_kind(seg)
            rows_i, shared = per_img.setdefault(r["image_id"], ([], {}))
            if kind == "polygons":
                row = len(rows_i)
                rows_i.append((kind, seg))
            else:
                note(r["image_id"], (int(seg["size"][0]), int(seg["size"][1])))
                if kind == "rle":
                    text = seg["counts"] if isinstance(seg["counts"], bytes) else seg["counts"].encode("ascii")
                    if text not in shared:
                        shared[text] = len(rows_i)
                        rows_i.append((kind, text))
                    row = shared[text]
                else:
                    row = len(rows_i)
                    rows_i.append((kind, np.asarray(seg["counts"], dtype=np.int64)))
            todo.append((r, row))
        size = {}
        for img in per_img:
            size[img] = seen.get(img, known.get(img))
            if size[img] is None:
                raise ValueError("image %r: a polygon segmentation needs the image's size (pass `images`, or an RLE record of that image)"
                                 % (img,))
            self._check_len(img, size[img][0] * size[img][1])
        counts, lengths, polys, psizes = [], [], [], []
        for img, (rows_i, _shared) in per_img.items():
            for kind, payload in rows_i:
                if kind == "polygons":
                    polys.append(payload)
                    psizes.append(size[img])
                else:
                    if kind == "counts" and (len(payload) == 0 or payload.min() < 0 or payload.max() >= 2 ** 32):
                        raise ValueError("image %r: uncompressed RLE counts must be non-negative run lengths" % (img,))
                    counts.append(rle_from_string(payload) if kind == "rle" else payload.astype(np.uint32))
                    lengths.append(size[img][0] * size[img][1])
        rrows, rarea = rle_to_bits(counts, lengths, self.device)
        prows, parea = poly_to_bits(polys, psizes, self.device)
        allrows, allarea = rrows + prows, torch.cat([rarea, parea])
        kr, kp, base = 0, len(rrows), {}
        for img, (rows_i, _shared) in per_img.items():
            idx = []
            for kind, _payload in rows_i:                            # row -> its place in the RLE launch or in the polygon launch
                if kind == "polygons":
                    idx.append(kp)
                    kp += 1
                else:
                    idx.append(kr)
                    kr += 1
            n = len(idx)
            if idx == list(range(idx[0], idx[0] + n)):
                area = allarea[idx[0]:idx[0] + n]
            else:                                                    # an image with rows from both launches
                area = allarea[torch.tensor(idx, dtype=torch.int64, device=allarea.device)]
            bits = torch.stack([allrows[j] for j in idx]) if n > 1 else allrows[idx[0]].reshape(1, -1)
            base[img] = side.add_chunk(img, bits, area, size[img][0] * size[img][1])
        known.update(seen)
        for r, row in todo:
            n = len(side.rec)
            side.rec.append((r["image_id"], r["category_id"], base[r["image_id"]] + row, float(r.get("score", 0.0)),
                             (r.get("area") if is_gt else None), int(r.get("iscrowd", 0)) if is_gt else 0,
                             int(r.get("ignore", 0)) if is_gt else 0, r.get("id", n + 1) if is_gt else n + 1))

    def _check_len(self, image_id, length):
        for s in (self._gt, self._dt):
            if s.length.get(image_id, length) != length:
                raise ValueError("image %r: masks of %d and of %d elements" % (image_id, s.length[image_id], length))

    def add_gt(self, records, images=None):
        """images: the sizes polygon records need -- COCO image dicts (id, height, width) or {image id: (h, w)}"""
        self._add_records(self._gt, records, True, images)

    def add_dt(self, records, images=None):
        self._add_records(self._dt, records, False, images)

    def _add_masks(self, side, image_id, masks, bits, category_id, rows, score, area, iscrowd, ignore, ids, is_gt):
        if bits is not None:
            words, marea, length = bits
            words, marea = words.contiguous(), marea.to(torch.int32)
            if words.dtype != torch.int64 or words.dim() != 2 or words.shape[1] != words_of(length) or not words.is_cuda:
                raise ValueError("bits: ((n, words_of(length)) CUDA int64 words, (n,) areas, length)")
        else:
            length = masks.shape[1]
            words, marea = pack_bits(masks)
        self._check_len(image_id, int(length))
        base = side.add_chunk(image_id, words, marea, length)
        cats = list(category_id)
        rows = list(range(len(cats))) if rows is None else [int(v) for v in rows]
        if rows and (min(rows) < 0 or max(rows) >= words.shape[0]):
            raise ValueError("rows must index the masks given")
        for j, c in enumerate(cats):
            n = len(side.rec)
            side.rec.append((image_id, int(c), base + rows[j], float(score[j]) if score is not None else 0.0,
                             (None if area is None else float(area[j])), int(iscrowd[j]) if iscrowd is not None else 0,
                             int(ignore[j]) if ignore is not None else 0, int(ids[j]) if ids is not None else n + 1))

    def add_gt_masks(self, image_id, masks, category_id, rows=None, area=None, iscrowd=None, ignore=None, ids=None, bits=None):
        """masks: (n, len) CUDA uint8 (or bits = (words, areas, len) from pack_bits); one record per entry of category_id, record j
        using mask rows[j] (default j)"""
        self._add_masks(self._gt, image_id, masks, bits, category_id, rows, None, area, iscrowd, ignore, ids, True)

    def add_dt_masks(self, image_id, masks, category_id, score, rows=None, bits=None):
        """detections from device masks: record j = (category_id[j], score[j]) on mask rows[j]; the C - 1 records that eval.py emits
        per predicted mask share one row, hence one row of the intersection matrix"""
        self._add_masks(self._dt, image_id, masks, bits, category_id, rows, score, None, None, None, None, False)

    # ---------------------------------------------------------------- evaluate ----------------------------------------------------------------
    def evaluate(self):
        """cocoeval.py:122-162: per (image, category | all, area range) matching at the largest maxDets, on the device"""
        p = self.params
        p.imgIds = sorted(set(p.imgIds))
        if p.useCats:
            p.catIds = sorted(set(p.catIds))
        p.maxDets = sorted(p.maxDets)
        p.iouThrs, p.recThrs = np.asarray(p.iouThrs, np.float64), np.asarray(p.recThrs, np.float64)
        T, A, I = len(p.iouThrs), len(p.areaRng), len(p.imgIds)
        K = len(p.catIds) if p.useCats else 1
        maxDet = p.maxDets[-1]
        img_index = {v: i for i, v in enumerate(p.imgIds)}
        cat_index = {v: i for i, v in enumerate(p.catIds)}
        dev = self.device

        def table(side):
            rec = [r for r in side.rec if r[0] in img_index and r[1] in cat_index]
            img = np.array([img_index[r[0]] for r in rec], np.int64)
            cat = np.array([cat_index[r[1]] for r in rec], np.int64)
            return rec, img, cat, np.array([r[2] for r in rec], np.int64)

        grec, gimg, gcat, grow = table(self._gt)
        drec, dimg, dcat, drow = table(self._dt)
        # mask areas of every image used: one copy for all of them
        def mask_areas(side):
            imgs = [v for v in p.imgIds if v in side.chunks]
            if not imgs:
                return {}, np.zeros((0,), np.int64)
            flat = torch.cat([a for v in imgs for (_b, a) in side.chunks[v]]).cpu().numpy().astype(np.int64)
            off, o = {}, 0
            for v in imgs:
                off[v] = o
                o += side.rows[v]
            return off, flat
        goff, gflat = mask_areas(self._gt)
        doff, dflat = mask_areas(self._dt)
        gm_area = np.array([gflat[goff[r[0]] + r[2]] for r in grec], np.int64)
        dm_area = np.array([dflat[doff[r[0]] + r[2]] for r in drec], np.int64)
        g_area = np.array([gm_area[j] if r[4] is None else r[4] for j, r in enumerate(grec)], np.float64)
        d_area = dm_area.astype(np.float64)                          # (loadRes: a detection's area is its mask's)
        dscore = np.array([r[3] for r in drec], np.float64)
        gk = gcat if p.useCats else np.zeros_like(gcat)
        dk = dcat if p.useCats else np.zeros_like(dcat)
        # cell order (k, image); inside a cell the reference's list order is (category, record)
        gord = np.lexsort((np.arange(len(grec)), gcat, gimg, gk))
        dord = np.lexsort((np.arange(len(drec)), dcat, -dscore, dimg, dk))     # stable: ties keep (category, record) order
        gcell, dcell = (gk * I + gimg)[gord], (dk * I + dimg)[dord]
        ncell = K * I
        Dfull = np.bincount(dcell, minlength=ncell).astype(np.int64)
        dstart = np.concatenate([[0], np.cumsum(Dfull)])
        rank = np.arange(len(dord)) - dstart[dcell]
        keep = rank < maxDet
        dord, dcell, rank = dord[keep], dcell[keep], rank[keep]
        Dc = np.bincount(dcell, minlength=ncell).astype(np.int64)
        Gc = np.bincount(gcell, minlength=ncell).astype(np.int64)
        dbeg, gbeg = np.concatenate([[0], np.cumsum(Dc)]), np.concatenate([[0], np.cumsum(Gc)])
        ND, NG = int(dbeg[-1]), int(gbeg[-1])
        gpos = np.arange(NG) - gbeg[gcell]

        # ---- pool of bit words + intersection jobs: every image with masks on both sides, all its distinct masks ----
        L = lib()
        parts, jobs, off, ooff, nblk = [], [], 0, 0, 0
        inter_off, inter_ld = np.zeros((I,), np.int64), np.ones((I,), np.int64)
        used = sorted(set(dimg[dord].tolist()) & set(gimg.tolist()))
        for i in used:
            v = p.imgIds[i]
            D, G, w = self._dt.rows[v], self._gt.rows[v], words_of(self._dt.length[v])
            if self._gt.length[v] != self._dt.length[v]:
                raise ValueError("image %r: ground truth and detections differ in size" % (v,))
            d_off = off
            for b, _a in self._dt.chunks[v]:
                parts.append(b.reshape(-1))
            off += D * w
            g_off = off
            for b, _a in self._gt.chunks[v]:
                parts.append(b.reshape(-1))
            off += G * w
            jobs.append((d_off, g_off, D, G, w, ooff, nblk, 0))
            inter_off[i], inter_ld[i] = ooff, G
            ooff += D * G
            nblk += int(L.rsis_mask_intersect_blocks(D, G, w))
        if nblk >= (1 << 31) - 1:
            raise ValueError("too many mask pairs for one launch")
        res = {"T": T, "A": A, "I": I, "K": K, "ND": ND, "NG": NG, "dbeg": dbeg, "gbeg": gbeg, "Dc": Dc, "Gc": Gc, "rank": rank,
               "dscore": dscore[dord], "drec": [drec[j] for j in dord], "grec": [grec[j] for j in gord], "maxDet": maxDet}
        cells_both = np.nonzero((Dc > 0) & (Gc > 0))[0]
        ioff = np.zeros((ncell + 1,), np.int64)
        ioff[1:] = np.cumsum(np.where((Dc > 0) & (Gc > 0), Dc * Gc, 0))
        NIOU = int(ioff[-1])
        dt = lambda a, t=torch.int64: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(t)
        ious_d = torch.zeros((max(NIOU, 1),), dtype=torch.float64, device=dev)
        if jobs and len(cells_both):
            pool = torch.cat(parts)
            jd = dt(np.array(jobs, np.int64))
            inter = torch.empty((ooff,), dtype=torch.int32, device=dev)
            check(L.rsis_mask_intersect_batch(ptr(pool), pool.numel(), ptr(jd), len(jobs), nblk, ptr(inter), ooff, stream()),
                  "rsis_mask_intersect_batch")
            ci = cells_both % I
            ctab = np.stack([dbeg[cells_both], Dc[cells_both], gbeg[cells_both], Gc[cells_both], inter_off[ci], inter_ld[ci],
                             ioff[cells_both], np.zeros_like(ci)], axis=1)
            cd = dt(ctab)
            a_dr, a_dm = dt(drow[dord], torch.int32), dt(dm_area[dord], torch.int32)
            a_gc, a_gm = dt(grow[gord], torch.int32), dt(gm_area[gord], torch.int32)
            a_cr = dt(np.array([grec[j][5] for j in gord], np.int64), torch.int32)
            check(L.rsis_coco_iou_batch(ptr(cd), len(ctab), ptr(inter), ooff, ptr(a_dr), ptr(a_dm), ND, ptr(a_gc), ptr(a_gm), ptr(a_cr), NG,
                                        ptr(ious_d), NIOU, stream()), "rsis_coco_iou_batch")
            res["inter"] = inter
            if self.keep_intersect_inputs:
                res["intersect_inputs"] = (pool, jd, len(jobs), nblk, ooff)
        # ---- matching cells (area range, k, image): ground truth in ignored-last order ----
        arng = np.asarray(p.areaRng, np.float64).reshape(A, 2)
        g_ign = np.array([grec[j][6] for j in gord], np.int64)
        g_crowd = np.array([grec[j][5] for j in gord], np.int64)
        ga = g_area[gord]
        gperm, gflag = np.zeros((A * NG,), np.int64), np.zeros((A * NG,), np.int64)
        for a in range(A):
            ig = ((g_ign != 0) | (ga < arng[a, 0]) | (ga > arng[a, 1])).astype(np.int64)
            o = np.lexsort((gpos, ig, gcell))                        # stable inside a cell
            gperm[a * NG:(a + 1) * NG] = gpos[o]
            gflag[a * NG:(a + 1) * NG] = ig[o] | (g_crowd[o] << 1)
        live = np.nonzero((Dc > 0) | (Gc > 0))[0]
        mt = []
        for a in range(A):
            mt.append(np.stack([ioff[live], Dc[live], Gc[live], dbeg[live], a * NG + gbeg[live], a * ND + dbeg[live], a * NG + gbeg[live],
                                np.full_like(live, a)], axis=1))
        res.update(gperm=gperm.reshape(A, NG), gflag=gflag.reshape(A, NG), live=live)
        dtm = torch.zeros((max(A * ND, 1), T), dtype=torch.int32, device=dev)
        dti = torch.zeros((max(A * ND, 1), T), dtype=torch.int32, device=dev)
        gtm = torch.zeros((max(A * NG, 1), T), dtype=torch.int32, device=dev)
        if len(live):
            mtab = np.concatenate(mt, axis=0)
            # cells with D == 0 or G == 0 hold no IoUs: their offset is not read
            md = dt(mtab)
            a_gp, a_gf = dt(gperm, torch.int32), dt(gflag, torch.int32)
            a_da = dt(d_area[dord], torch.float64)
            a_ar, a_th = dt(arng, torch.float64), dt(p.iouThrs, torch.float64)
            check(L.rsis_coco_match_batch(ptr(md), len(mtab), ptr(ious_d) if NIOU else None, NIOU, ptr(a_gp) if NG else None,
                                          ptr(a_gf) if NG else None, A * NG, ptr(a_da) if ND else None, ND, ptr(a_ar), A, ptr(a_th), T,
                                          ptr(dtm) if ND else None, ptr(dti) if ND else None, A * ND, ptr(gtm) if NG else None, A * NG,
                                          stream()), "rsis_coco_match_batch")
        res["dtm"] = dtm.cpu().numpy()[:A * ND].reshape(A, ND, T)
        res["dti"] = dti.cpu().numpy()[:A * ND].reshape(A, ND, T)
        res["gtm"] = gtm.cpu().numpy()[:A * NG].reshape(A, NG, T)
        res["ious"] = ious_d.cpu().numpy()[:NIOU]
        res["ioff"] = ioff
        self._res = res
        self._evalImgs = None
        self.eval = {}
        return self

    # views of the device results in the reference's form (tests, inspection); not needed by accumulate()
    def iou_matrix(self, image_id, category_id=-1):
        """self.ious[imgId, catId] of the reference: (D, G) float64, detections in score order (truncated), ground truth in list order"""
        r, p = self._res, self.params
        k = p.catIds.index(category_id) if p.useCats else 0
        c = k * r["I"] + p.imgIds.index(image_id)
        D, G = int(r["Dc"][c]), int(r["Gc"][c])
        if D == 0 or G == 0:
            return np.zeros((D, G)) if (D or G) else []
        return r["ious"][r["ioff"][c]:r["ioff"][c] + D * G].reshape(D, G)

    @property
    def evalImgs(self):
        """list over [category][area range][image] of the reference's per-cell dicts (None for a cell without masks)"""
        if self._evalImgs is None:
            r, p = self._res, self.params
            out = []
            gid = np.array([g[7] for g in r["grec"]], np.int64)
            did = np.array([d[7] for d in r["drec"]], np.int64)
            for k in range(r["K"]):
                for a in range(r["A"]):
                    for i in range(r["I"]):
                        c = k * r["I"] + i
                        D, G = int(r["Dc"][c]), int(r["Gc"][c])
                        if D == 0 and G == 0:
                            out.append(None)
                            continue
                        ds, gs = slice(r["dbeg"][c], r["dbeg"][c] + D), slice(r["gbeg"][c], r["gbeg"][c] + G)
                        gids = gid[gs][r["gperm"][a, gs]]
                        dids = did[ds]
                        dm, gm = r["dtm"][a, ds].T, r["gtm"][a, gs].T
                        out.append({"image_id": p.imgIds[i], "category_id": p.catIds[k] if p.useCats else -1, "aRng": list(p.areaRng[a]),
                                    "maxDet": r["maxDet"], "dtIds": dids.tolist(), "gtIds": gids.tolist(),
                                    "dtMatches": np.where(dm > 0, np.concatenate([[0], gids])[dm], 0).astype(np.float64),
                                    "gtMatches": np.where(gm > 0, np.concatenate([[0], dids])[gm], 0).astype(np.float64),
                                    "dtScores": r["dscore"][ds].tolist(), "gtIgnore": (r["gflag"][a, gs] & 1),
                                    "dtIgnore": r["dti"][a, ds].T.astype(bool)})
            self._evalImgs = out
        return self._evalImgs

    # --------------------------------------------------------------- accumulate ---------------------------------------------------------------
    def accumulate(self):
        """cocoeval.py:316-415 from the device results"""
        r, p = self._res, self.params
        if r is None:
            raise Exception("Please run evaluate() first")
        I = r["I"]
        per_k = []
        for k in range(r["K"]):
            d0, d1 = int(r["dbeg"][k * I]), int(r["dbeg"][(k + 1) * I])
            g0, g1 = int(r["gbeg"][k * I]), int(r["gbeg"][(k + 1) * I])
            cells = bool(((r["Dc"][k * I:(k + 1) * I] > 0) | (r["Gc"][k * I:(k + 1) * I] > 0)).any())
            per_k.append({"cells": cells, "scores": r["dscore"][d0:d1], "rank": r["rank"][d0:d1],
                          "dtm": [r["dtm"][a, d0:d1] for a in range(r["A"])], "dti": [r["dti"][a, d0:d1] for a in range(r["A"])],
                          "gig": [r["gflag"][a, g0:g1] & 1 for a in range(r["A"])]})
        precision, recall = accumulate_cells(per_k, p.maxDets, p.recThrs, r["T"], r["A"])
        self.eval = {"params": p, "counts": [r["T"], len(p.recThrs), r["K"], r["A"], len(p.maxDets)], "precision": precision, "recall": recall}
        return self

    def summarize(self, out=None):
        """cocoeval.py:417-489: the reference copy's 13 stats, printed in its format"""
        if not self.eval:
            raise Exception("Please run accumulate() first")
        self.stats = summarize_stats(self.eval["precision"], self.eval["recall"], self.params, out or sys.stdout)
        return self.stats


def accumulate_cells(per_k, maxDets, recThrs, T, A):
    """The arithmetic of cocoeval.py:335-406.  per_k[k]: 'cells' (any image of this category has masks), and concatenated over its
    images in image order: 'scores' (n,), 'rank' (n,: position of the detection in its image's score order), per area range a
    'dtm'[a] / 'dti'[a] (n, T) match / ignore flags, 'gig'[a] (g,) ground-truth ignore flags."""
    R, K, M = len(recThrs), len(per_k), len(maxDets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, ck in enumerate(per_k):
        if not ck["cells"]:
            continue
        for m, maxDet in enumerate(maxDets):
            sel = ck["rank"] < maxDet
            inds = np.argsort(-ck["scores"][sel], kind="mergesort")
            for a in range(A):
                dtm = ck["dtm"][a][sel][inds].T
                dtIg = ck["dti"][a][sel][inds].T
                npig = np.count_nonzero(ck["gig"][a] == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    q = np.zeros((R,))
                    if nd:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]   # right-to-left running maximum
                        pi = np.searchsorted(rc, recThrs, side="left")
                        ok = pi < nd                                 # (the reference stops filling at the first index past the end)
                        q[ok] = pr[pi[ok]]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize_stats(precision, recall, p, out=sys.stdout):
    """cocoeval.py:422-468 (_summarize / _summarizeDets): 13 numbers, selected by EQUALITY on maxDets and on iouThrs"""
    iouThrs = np.asarray(p.iouThrs)

    def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
        iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        titleStr = 'Average Precision' if ap == 1 else 'Average Recall'
        typeStr = '(AP)' if ap == 1 else '(AR)'
        iouStr = '{:0.2f}:{:0.2f}'.format(iouThrs[0], iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
        aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
        s = precision if ap == 1 else recall
        if iouThr is not None:
            s = s[np.where(iouThr == iouThrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        print(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s), file=out)
        return mean_s

    md = p.maxDets
    if len(md) < 3:
        raise ValueError("summarize needs three maxDets (cocoeval.py:456-467 indexes maxDets[0..2])")
    stats = np.zeros((13,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5, maxDets=md[2])
    stats[2] = _summarize(1, iouThr=.6, maxDets=md[2])
    stats[3] = _summarize(1, iouThr=.7, maxDets=md[2])
    stats[4] = _summarize(1, iouThr=.75, maxDets=md[2])
    stats[5] = _summarize(1, iouThr=.8, maxDets=md[2])
    stats[6] = _summarize(1, maxDets=md[1])
    stats[7] = _summarize(0, maxDets=md[1])
    stats[8] = _summarize(1, iouThr=.5, maxDets=md[0])
    stats[9] = _summarize(1, iouThr=.5, maxDets=md[1])
    stats[10] = _summarize(0, iouThr=.5, maxDets=md[1])
    stats[11] = _summarize(0, iouThr=.7, maxDets=md[1])
    stats[12] = _summarize(0, iouThr=.85, maxDets=md[1])
    return stats


def run_reference_protocol(ev, img_ids, cat_ids, max_dets, use_cats, all_classes, class_names=None, out=None):
    """reference eval.py:379-398 on a COCOEvalDevice: maxDets = [1, -max_dets, 100], all classes together, then (with --all_classes)
    one category at a time.  Returns {'stats': [...], 'per_class': {category: [...]}}"""
    out = out or sys.stdout
    ev.params.maxDets = [1, max_dets, 100]
    ev.params.useCats = 1 if use_cats else 0
    ev.params.imgIds = sorted(img_ids)
    ev.params.catIds = list(cat_ids)
    print("Results for all the classes together", file=out)
    ev.evaluate().accumulate().summarize(out)
    res = {"stats": [float(v) for v in ev.stats], "per_class": {}}
    if all_classes:
        for c in list(cat_ids):
            print("Testing class dataset_id: " + str(c), file=out)
            if class_names is not None:
                print("Which corresponds to name: " + str(class_names[c]), file=out)
            ev.params.catIds = [c]
            ev.evaluate().accumulate().summarize(out)
            res["per_class"][str(c)] = [float(v) for v in ev.stats]
        ev.params.catIds = list(cat_ids)
    return res


def get_cli_parser():
    ap = argparse.ArgumentParser(prog="python -m rsis_amd.cocoeval", description="COCO segm AP of a predictions file against a "
                                 "ground-truth file, on the GPU (both: JSON lists of COCO records, or COCO dicts with 'annotations' and "
                                 "'images'; segmentations as compressed RLE, uncompressed RLE or polygons)")
    ap.add_argument("--gt", required=True, help="ground truth: JSON list of annotation records, or a COCO dict with 'annotations'")
    ap.add_argument("--dt", required=True, help="detections: a *_predictions.json of rsis_amd.eval or of the reference's eval.py")
    ap.add_argument("-max_dets", dest="max_dets", default=100, type=int)
    ap.add_argument("--ignore_cats", dest="use_cats", action="store_false")
    ap.add_argument("--all_classes", dest="all_classes", action="store_true")
    ap.add_argument("--all_images", dest="all_images", action="store_true", help="evaluate every image the ground-truth file lists "
                    "under 'images' (also those without annotations), not only the images that have ground-truth records")
    ap.add_argument("--out", default=None, help="write the stats as JSON here")
    return ap


def load_coco_file(path):
    """a JSON list of records -> (records, None); a COCO dict -> (its 'annotations', its 'images' or None)"""
    with open(path) as f:
        d = json.load(f)
    if isinstance(d, dict):
        return d["annotations"], d.get("images")
    return d, None


def main(argv=None):
    a = get_cli_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rsis_amd.cocoeval needs the GPU: the HIP library is the only compute path")
    (gt, images), (dt, _) = load_coco_file(a.gt), load_coco_file(a.dt)
    if a.all_images and not images:
        raise SystemExit("--all_images needs a ground-truth file with an 'images' list")
    ev = COCOEvalDevice(gt, dt, images=images)
    img_ids = sorted(_image_sizes(images)) if a.all_images else sorted(set(r["image_id"] for r in gt))
    res = run_reference_protocol(ev, img_ids, sorted(set(r["category_id"] for r in gt)), a.max_dets,
                                 a.use_cats, a.all_classes)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f)
    return res


if __name__ == "__main__":
    main()
