"""Cityscapes instance-level measures (AP, AP50% per class) of a results folder -- what the paper's Cityscapes table took from the
benchmark's `evalInstanceLevelSemanticLabeling` script for the `<sample>.txt` + mask PNGs that `rsis_amd.eval_cityscapes` writes.  The
pixel counting runs on the device (two grouped launches of rsis_amd/csrc/insteval.hip: which ids occur, then the joint counts of all
masks against the id image); matching, accumulation and AP are numpy float64 on the host.

    python -m rsis_amd.cityscapes_eval --results DIR --gt DIR [--json OUT]

RESTATED, NOT COMPARED AGAINST THE OFFICIAL SCRIPT: `cityscapesscripts` is not part of this project's environment, so the definition
below was written down from memory of that script and is checked only against an independent slow statement of the same text
(tests/cityscapes_golden.py).

  * Evaluated classes CLASS_IDS = 24, 25, 26, 27, 28, 31, 32, 33 (person, rider, car, truck, bus, train, motorcycle, bicycle).  Void
    ids VOID_IDS = 0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30; the void mask is isin(gt, VOID_IDS) on the RAW 16-bit values, so
    a caravan *instance* (29001) is not void.
  * Ground truth of an image: every distinct value v of `*_gtFine_instanceIds.png` is an instance with labelID = v if v < 1000 else
    v // 1000 and its pixel count; it belongs to class labelID if that is an evaluated class.  Values below 1000 of an evaluated class
    are group regions.
  * Predictions of an image: the lines `<relative png> <labelID> <confidence>` of its .txt, paths relative to the txt's folder.  A line
    of a non-evaluated class is skipped, a mask with no non-zero pixel is skipped, a mask of another size than the ground truth is an
    error.  pixelCount = non-zero pixels, voidIntersection = non-zero pixels on void; every ground-truth instance of the same class
    (groups included) with a non-empty intersection is recorded with that intersection.
  * Thresholds np.arange(0.5, 1.0, 0.05) (float64, those ten values); one minimum region size, 100 pixels; no distance criteria.
  * Per (class, threshold), image by image: the ground truths are those with instID >= 1000 and pixelCount >= 100.  Each starts as
    (true = 1, score = -inf, unmatched); for each recorded prediction with intersection / (gt.pixelCount + pred.pixelCount -
    intersection) > threshold (float64, strict) the first sets matched and the score, each further one keeps the larger confidence on
    the ground truth and appends the smaller as (true = 0).  A ground truth without any is one hard false negative and is dropped.
    Then each prediction with no ground truth (groups and small ones included) above the threshold: ignore = voidIntersection + its
    intersections with group regions (instID < 1000) + its intersections with ground truths smaller than 100 pixels (two sums: a
    group region below 100 pixels adds twice); it is appended as (true = 0, its confidence) only if ignore / pixelCount <= threshold.
    haveGt / havePred: some image has a non-empty filtered ground-truth list / prediction list of the class.
  * AP of a (class, threshold): NaN without ground truth, 0 with ground truth and no prediction (or with both and empty lists), else: sort by score ascending,
    cumulative sum of `true`, one operating point per DISTINCT score at its first index k (below = trues before k): tp = total_true -
    below, fp = n - k - tp, fn = below + hardFns, precision = tp / (tp + fp), recall = tp / (tp + fn); a last point (1, 0);
    AP = dot(precision, convolve([recall[0]] + recall + [0], [-0.5, 0, 0.5], 'valid')).  Tied scores share one point, so the order
    of the sort among ties cannot matter.
  * Averages: allAp = nanmean over classes and thresholds, allAp50% over classes at 0.5, per class ap (mean over thresholds) / ap50%.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

from ._lib import _device, check, lib, ptr, stream

CLASS_IDS = (24, 25, 26, 27, 28, 31, 32, 33)                  # == eval_post.CITYSCAPES_CLASS_IDS
CLASS_NAMES = ("person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")
VOID_IDS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)
THRESHOLDS = np.arange(0.5, 1.0, 0.05)
MIN_REGION = 100
GT_SUFFIX = "_gtFine_instanceIds.png"
JOB = 16                                                       # int64 entries per job (include/rsis_hip.h)


# ------------------------------------------------------------------ the two launches ------------------------------------------------------------------
def _gt_bytes(g, what, device):
    """2-d image of ids 0 .. 65535 (numpy or tensor, any integer type) -> flat uint8 tensor of its little-endian uint16 values"""
    if isinstance(g, torch.Tensor):
        if g.dim() != 2 or g.numel() < 1 or g.dtype.is_floating_point:
            raise ValueError("%s: an id image is a non-empty 2-d integer tensor (got %s %s)" % (what, g.dtype, tuple(g.shape)))
        v = g.to(torch.int32)
        if int(v.min()) < 0 or int(v.max()) > 65535:
            raise ValueError("%s: ids outside 0 .. 65535" % what)
        v = torch.where(v > 32767, v - 65536, v).to(torch.int16).contiguous()
        return v.view(-1).view(torch.uint8), tuple(g.shape)
    a = np.asarray(g)
    if a.ndim != 2 or a.size < 1 or a.dtype.kind not in "iu":
        raise ValueError("%s: an id image is a non-empty 2-d integer array (got %s %s)" % (what, a.dtype, a.shape))
    if a.dtype != np.uint16 and (a.min() < 0 or a.max() > 65535):
        raise ValueError("%s: ids outside 0 .. 65535" % what)
    return torch.from_numpy(np.ascontiguousarray(a.astype("<u2")).reshape(-1).view(np.uint8)), a.shape


def _pack_masks(m, shape, what, device):
    """(P, h, w) masks (zero / non-zero; numpy or tensor, bool or integer) -> (int64 device tensor of P * stride words, stride)"""
    npix = shape[0] * shape[1]
    stride = (npix + 63) // 64
    n = len(m)
    if n == 0:
        return torch.zeros((0,), dtype=torch.int64, device=device), stride
    if isinstance(m, torch.Tensor) and m.is_cuda:
        if tuple(m.shape[1:]) != tuple(shape):
            raise ValueError("%s: masks of size %s for a ground truth of %s" % (what, tuple(m.shape[1:]), tuple(shape)))
        bits = torch.empty((n * stride,), dtype=torch.int64, device=m.device)
        area = torch.empty((n,), dtype=torch.int32, device=m.device)
        flat = (m != 0).to(torch.uint8).reshape(n, npix).contiguous()
        for p0 in range(0, n, 65535):
            k = min(65535, n - p0)
            check(lib().rsis_mask_pack_bits(ptr(flat[p0:]), k, npix, ptr(bits[p0 * stride:]), stride, ptr(area[p0:]), stream()),
                  "rsis_mask_pack_bits")
        return bits.to(device), stride
    rows = []
    for k, one in enumerate(m):
        a = one.numpy() if isinstance(one, torch.Tensor) else np.asarray(one)
        if a.shape != tuple(shape):
            raise ValueError("%s: mask %d has size %s, the ground truth %s" % (what, k, a.shape, tuple(shape)))
        b = np.zeros((stride * 8,), np.uint8)
        pk = np.packbits(a.reshape(-1) != 0, bitorder="little")
        b[:pk.size] = pk
        rows.append(b)
    return torch.from_numpy(np.concatenate(rows).view("<u8").astype(np.int64, copy=False)).to(device), stride


def job_table(npix, P, S=None, align=2, strides=None):
    """The pool layout and the job table of a call: image j lies at byte gt_off of one pool (each start rounded up to `align` bytes,
    align even), its flags / lut at j * 65536, its masks at bits_off (P_j * stride_j words, back to back), its table at counts_off
    ((P_j + 1) * S_j counts, back to back).  Returns (jobs (N, 16) int64, pool bytes (a multiple of 16), overlap blocks, presence
    blocks, counts length)."""
    if align < 2 or align % 2:
        raise ValueError("align must be even")
    L = lib()
    jobs = np.zeros((len(npix), JOB), np.int64)
    off = bits = cnt = blk = pblk = 0
    for j, n in enumerate(npix):
        n, p = int(n), int(P[j])
        if n < 1 or n >= 1 << 32:
            raise ValueError("image %d: %d pixels (1 .. 2^32 - 1 are supported)" % (j, n))
        s = 1 if S is None else int(S[j])
        if s < 1 or s > 65535:
            raise ValueError("image %d: %d distinct ids (1 .. 65535 are supported)" % (j, s))
        stride = (n + 63) // 64 if strides is None else int(strides[j])
        off = -(-off // align) * align
        jobs[j, :10] = (off, n, j * 65536, bits, stride, p, s, cnt, blk, pblk)
        off += 2 * n
        bits += p * stride
        cnt += (p + 1) * s
        blk += int(L.rsis_inst_overlap_blocks(n, p))
        pblk += int(L.rsis_inst_overlap_blocks(n, 0))
    return jobs, (off + 15) // 16 * 16, blk, pblk, cnt


def overlap_counts_batch(gt_images, mask_sets, device="cuda", align=2, lead=0):
    """lists of N id images (h, w) and N mask sets (P_j, h, w) -> list of N (counts, ids): ids = the sorted distinct values of the image
    (int64, S), counts (P_j + 1, S) int64 host array, counts[p, s] = non-zero pixels of mask p on ids[s], last row = pixels of ids[s].
    One host -> device copy of the pool, the presence launch, the lut (device), the overlap launch, one copy back.  `lead` bytes
    (even) are left free in front of the first image (tests: images at odd pool positions)."""
    device = _device(device, "rsis_amd.cityscapes_eval")
    if len(gt_images) != len(mask_sets):
        raise ValueError("%d id images for %d mask sets" % (len(gt_images), len(mask_sets)))
    n = len(gt_images)
    if n == 0:
        return []
    L = lib()
    gts = [_gt_bytes(g, "gt[%d]" % j, device) for j, g in enumerate(gt_images)]
    packed = [_pack_masks(m, shp, "masks[%d]" % j, device) for j, (m, (_b, shp)) in enumerate(zip(mask_sets, gts))]
    npix = [shp[0] * shp[1] for _b, shp in gts]
    P = [len(m) for m in mask_sets]
    jobs, length, _blk, pblk, _cnt = job_table(npix, P, None, align)
    if lead:
        if lead % 2:
            raise ValueError("lead must be even")
        jobs[:, 0] += lead
        length = (length + lead + 15) // 16 * 16
    on_host = all(not b.is_cuda for b, _s in gts)
    pool = torch.zeros((length,), dtype=torch.uint8, device="cpu" if on_host else device)
    for (b, _s), J in zip(gts, jobs):
        pool[J[0]:J[0] + 2 * J[1]] = b.to(pool.device)
    pool = pool.to(device)
    djobs = torch.from_numpy(jobs).to(device)
    flags = torch.empty((n * 65536,), dtype=torch.uint8, device=device)
    check(L.rsis_inst_presence_batch(ptr(pool), pool.numel(), ptr(djobs), n, pblk, ptr(flags), flags.numel(), stream()),
          "rsis_inst_presence_batch")
    present = flags.view(n, 65536) != 0
    slot = present.to(torch.int32).cumsum(1) - 1                                      # id -> slot in ascending id order
    slot = torch.where(present, slot, torch.full_like(slot, 65535))                   # (65535: never a slot, S <= 65535)
    lut = torch.where(slot > 32767, slot - 65536, slot).to(torch.int16).contiguous().view(-1)
    present_h = present.cpu().numpy()                                                 # (the one sync of the call: S sizes the tables)
    ids = [np.flatnonzero(r).astype(np.int64) for r in present_h]
    S = [len(v) for v in ids]
    if max(S) > 65535:
        raise ValueError("an image with all 65536 ids present is not supported")
    jobs2, _length, blk, _pblk, cnt = job_table(npix, P, S, align)
    jobs2[:, 0] = jobs[:, 0]
    djobs = torch.from_numpy(jobs2).to(device)
    bits = torch.cat([b for b, _st in packed]) if sum(P) else torch.zeros((0,), dtype=torch.int64, device=device)
    counts = torch.empty((cnt,), dtype=torch.int32, device=device)
    check(L.rsis_inst_overlap_batch(ptr(pool), pool.numel(), ptr(djobs), n, blk, ptr(lut), lut.numel(), ptr(bits) if bits.numel() else None,
                                    bits.numel(), ptr(counts), counts.numel(), stream()), "rsis_inst_overlap_batch")
    ch = counts.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return [(ch[J[7]:J[7] + (p + 1) * s].reshape(p + 1, s), v) for J, p, s, v in zip(jobs2, P, S, ids)]


def overlap_counts(gt_ids, masks, device="cuda"):
    """one id image (h, w) and its P masks (P, h, w), device tensors or numpy -> (counts (P + 1, S) int64, ids (S,) int64), see
    overlap_counts_batch"""
    return overlap_counts_batch([gt_ids], [masks], device)[0]


# ------------------------------------------------------------------ the measure (host, float64) ------------------------------------------------------------------
def label_of(inst_id):
    return inst_id if inst_id < 1000 else inst_id // 1000


def assign(counts, ids, pred_labels, pred_scores):
    """The match lists of one image.  counts (Q + 1, S): row q = the pixels of prediction q per id, last row = the histogram of ids (S,);
    pred_labels / pred_scores: the Q lines of the .txt.  Returns a dict of arrays:
      gt    (G, 3) int64 : instID, labelID, pixelCount of every id of an evaluated class, ascending instID
      pred  (K, 4) int64 : line index, labelID, pixelCount, voidIntersection of every kept prediction, in line order
      conf  (K,) float64 : their confidences
      pairs (M, 3) int64 : (row of pred, row of gt, intersection) of every same-class pair with a non-empty intersection, by pred, gt"""
    counts = np.asarray(counts, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    labels = np.where(ids < 1000, ids, ids // 1000)
    is_inst = np.isin(labels, CLASS_IDS)
    gsel = np.flatnonzero(is_inst)
    gt = np.stack([ids[gsel], labels[gsel], counts[-1, gsel]], 1).reshape(-1, 3)
    void = np.isin(ids, VOID_IDS)
    pred, conf, pairs = [], [], []
    for q, (lab, sc) in enumerate(zip(pred_labels, pred_scores)):
        lab = int(lab)
        if lab not in CLASS_IDS:
            continue
        row = counts[q]
        area = int(row.sum())
        if area == 0:
            continue
        k = len(pred)
        pred.append((q, lab, area, int(row[void].sum())))
        conf.append(float(sc))
        for g in np.flatnonzero((gt[:, 1] == lab) & (row[gsel] > 0)):
            pairs.append((k, int(g), int(row[gsel[g]])))
    return {"gt": gt.astype(np.int64), "pred": np.array(pred, np.int64).reshape(-1, 4), "conf": np.array(conf, np.float64),
            "pairs": np.array(pairs, np.int64).reshape(-1, 3)}


def match_lists(images, class_id, threshold):
    """(y_true, y_score, hardFns, haveGt, havePred) of one (class, threshold) over the images' `assign` records"""
    y_true, y_score, hard = [], [], 0
    have_gt = have_pred = False
    for im in images:
        gt, pred, conf, pairs = im["gt"], im["pred"], im["conf"], im["pairs"]
        grow = np.flatnonzero((gt[:, 1] == class_id) & (gt[:, 0] >= 1000) & (gt[:, 2] >= MIN_REGION))
        prow = np.flatnonzero(pred[:, 1] == class_id)
        have_gt |= len(grow) > 0
        have_pred |= len(prow) > 0
        if len(pairs):
            inter = pairs[:, 2].astype(np.float64)
            iou = inter / (gt[pairs[:, 1], 2] + pred[pairs[:, 0], 2] - pairs[:, 2]).astype(np.float64)
            over = iou > threshold
        else:
            over = np.zeros((0,), bool)
        for g in grow:
            matched, score = False, -np.inf
            for k in pairs[over & (pairs[:, 1] == g), 0]:
                c = conf[k]
                if matched:
                    y_true.append(0.0)
                    y_score.append(min(score, c))
                    score = max(score, c)
                else:
                    matched, score = True, c
            if not matched:
                hard += 1
                continue
            y_true.append(1.0)
            y_score.append(score)
        group, small = gt[:, 0] < 1000, gt[:, 2] < MIN_REGION
        for k in prow:
            mine = pairs[:, 0] == k
            if (mine & over).any():
                continue
            ignore = int(pred[k, 3]) + int(pairs[mine & group[pairs[:, 1]], 2].sum()) + int(pairs[mine & small[pairs[:, 1]], 2].sum())
            if float(ignore) / float(pred[k, 2]) <= threshold:
                y_true.append(0.0)
                y_score.append(conf[k])
    return np.array(y_true, np.float64), np.array(y_score, np.float64), hard, bool(have_gt), bool(have_pred)


def average_precision(y_true, y_score, hard_fns):
    """the AP of one (class, threshold) from its lists (module docstring); the lists are not empty"""
    order = np.argsort(y_score, kind="stable")
    ys, yt = np.asarray(y_score, np.float64)[order], np.asarray(y_true, np.float64)[order]
    cum = np.cumsum(yt)
    _v, first = np.unique(ys, return_index=True)
    n, total = len(ys), cum[-1]
    below = np.where(first > 0, cum[first - 1], 0.0)
    tp = total - below
    fp = n - first - tp
    fn = below + hard_fns
    precision = np.append(tp / (tp + fp), 1.0)
    recall = np.append(tp / (tp + fn), 0.0)
    rc = np.concatenate([[recall[0]], recall, [0.0]])
    return float(np.dot(precision, np.convolve(rc, [-0.5, 0.0, 0.5], "valid")))


def evaluate_matches(images):
    """list of per-image `assign` records -> (8, 10) float64 array of AP per (class, threshold)"""
    aps = np.zeros((len(CLASS_IDS), len(THRESHOLDS)), np.float64)
    for ci, cid in enumerate(CLASS_IDS):
        for ti, th in enumerate(THRESHOLDS):
            y_true, y_score, hard, have_gt, have_pred = match_lists(images, cid, th)
            if have_gt and have_pred and len(y_true):
                aps[ci, ti] = average_precision(y_true, y_score, hard)
            elif have_gt:
                aps[ci, ti] = 0.0
            else:
                aps[ci, ti] = np.nan
    return aps


def compute_averages(aps):
    """(8, 10) AP array -> {"allAp", "allAp50%", "classes": {name: {"ap", "ap50%"}}}; a class without ground truth is NaN and left out of
    the means (all NaN: NaN)"""
    aps = np.asarray(aps, np.float64)

    def nanmean(a):
        a = a[~np.isnan(a)]
        return float(a.mean()) if a.size else float("nan")
    out = {"allAp": nanmean(aps), "allAp50%": nanmean(aps[:, 0]), "classes": {}}
    for ci, name in enumerate(CLASS_NAMES):
        out["classes"][name] = {"ap": float(np.mean(aps[ci])), "ap50%": float(aps[ci, 0])}
    return out


# ------------------------------------------------------------------ files ------------------------------------------------------------------
def read_gt_png(path):
    """16-bit greyscale PNG -> (h, w) uint16 array; anything else is refused"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("I;16", "I;16B", "I;16L", "I"):
            raise ValueError("%s: mode %r is not an instance-id image: 16-bit greyscale only (8-bit and RGB files are refused)" % (path, im.mode))
        a = np.array(im)
    if a.ndim != 2 or a.min() < 0 or a.max() > 65535:
        raise ValueError("%s: decoded as %s %s, not as 16-bit ids" % (path, a.dtype, a.shape))
    return a.astype(np.uint16)


def read_mask_png(path):
    """prediction mask: any single-channel PNG, non-zero = set -> (h, w) uint8 0 / 1"""
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im)
    if a.ndim != 2:
        raise ValueError("%s: a prediction mask has one channel (decoded as %s)" % (path, a.shape))
    return (a != 0).astype(np.uint8)


def parse_result_txt(path):
    """-> list of (absolute png path, labelID, confidence) of the lines of a result .txt; blank lines are skipped"""
    out, base = [], os.path.dirname(os.path.abspath(path))
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 3:
                raise ValueError("%s:%d: expected `<png> <labelID> <confidence>`, got %r" % (path, no, line.rstrip("\n")))
            if os.path.isabs(parts[0]):
                raise ValueError("%s:%d: the mask path must be relative to the txt's folder" % (path, no))
            try:
                out.append((os.path.join(base, parts[0]), int(parts[1]), float(parts[2])))
            except ValueError:
                raise ValueError("%s:%d: labelID / confidence are not numbers: %r" % (path, no, line.rstrip("\n")))
    return out


def pair_files(results_dir, gt_dir):
    """-> sorted list of (stem, txt path, ground-truth path): `<stem>.txt` of results_dir with the file anywhere under gt_dir named
    <stem without a trailing _leftImg8bit> + _gtFine_instanceIds.png"""
    gts = {}
    for root, _dirs, files in os.walk(gt_dir):
        for f in files:
            if f.endswith(GT_SUFFIX):
                if f in gts:
                    raise ValueError("two ground-truth files named %s under %s" % (f, gt_dir))
                gts[f] = os.path.join(root, f)
    out = []
    for f in sorted(os.listdir(results_dir)):
        if not f.endswith(".txt"):
            continue
        stem = f[:-4]
        key = (stem[:-len("_leftImg8bit")] if stem.endswith("_leftImg8bit") else stem) + GT_SUFFIX
        if key not in gts:
            raise ValueError("%s: no ground truth %s under %s" % (f, key, gt_dir))
        out.append((stem, os.path.join(results_dir, f), gts[key]))
    if not out:
        raise ValueError("no result .txt under %s" % results_dir)
    return out


def score_image_sets(gt_images, mask_sets, rows, labels, scores, counts_fn=None):
    """the `assign` records of a batch: image j has the DISTINCT masks mask_sets[j]; its line q uses mask rows[j][q] (-1: a line whose
    mask was not needed) with labels[j][q] / scores[j][q]"""
    res = (counts_fn or overlap_counts_batch)(gt_images, mask_sets)
    out = []
    for (counts, ids), r, lab, sc in zip(res, rows, labels, scores):
        r = np.asarray(r, np.int64).reshape(-1)
        full = np.zeros((len(r) + 1, counts.shape[1]), np.int64)
        full[:-1][r >= 0] = counts[r[r >= 0]]
        full[-1] = counts[-1]
        out.append(assign(full, ids, lab, sc))
    return out


def evaluate_dirs(results_dir, gt_dir, batch=16, counts_fn=None):
    """every `<stem>.txt` of results_dir against its ground truth under gt_dir -> {"aps": (8, 10) array, "averages": compute_averages,
    "images": n}.  Each distinct mask file (by content) of an image is decoded and counted once; `batch` images go to the device in one
    pool."""
    files = pair_files(results_dir, gt_dir)
    records = []
    for b0 in range(0, len(files), batch):
        gt_images, mask_sets, rows, labels, scores = [], [], [], [], []
        for _stem, txt, gtf in files[b0:b0 + batch]:
            g = read_gt_png(gtf)
            seen, masks, r, lab, sc = {}, [], [], [], []
            for png, label, confidence in parse_result_txt(txt):
                lab.append(label)
                sc.append(confidence)
                if label not in CLASS_IDS:
                    r.append(-1)
                    continue
                with open(png, "rb") as f:
                    key = hashlib.sha1(f.read()).digest()
                if key not in seen:
                    m = read_mask_png(png)
                    if m.shape != g.shape:
                        raise ValueError("%s: mask of size %s for a ground truth of %s (%s)" % (png, m.shape, g.shape, gtf))
                    seen[key] = len(masks)
                    masks.append(m)
                r.append(seen[key])
            gt_images.append(g)
            mask_sets.append(masks)
            rows.append(r)
            labels.append(lab)
            scores.append(sc)
        records += score_image_sets(gt_images, mask_sets, rows, labels, scores, counts_fn)
    aps = evaluate_matches(records)
    return {"aps": aps, "averages": compute_averages(aps), "images": len(files)}


def _f(v):
    return "  nan" if np.isnan(v) else "%5.3f" % v


def summary(averages):
    """the text table: one row per class (AP, AP50%), then the averages"""
    lines = ["%-15s %7s %7s" % ("what", "AP", "AP50%"), "-" * 31]
    for name in CLASS_NAMES:
        c = averages["classes"][name]
        lines.append("%-15s %7s %7s" % (name, _f(c["ap"]), _f(c["ap50%"])))
    lines += ["-" * 31, "%-15s %7s %7s" % ("average", _f(averages["allAp"]), _f(averages["allAp50%"]))]
    return "\n".join(lines) + "\n"


def write_result_json(path, result):
    """{"averages": ..., "aps": 8 x 10 list, "thresholds", "classes", "images"} with NaN written as null; returns the file name"""
    clean = lambda v: None if isinstance(v, float) and np.isnan(v) else v
    av = result["averages"]
    doc = {"averages": {"allAp": clean(av["allAp"]), "allAp50%": clean(av["allAp50%"]),
                        "classes": {k: {m: clean(x) for m, x in c.items()} for k, c in av["classes"].items()}},
           "aps": [[clean(float(x)) for x in r] for r in np.asarray(result["aps"])],
           "thresholds": [float(t) for t in THRESHOLDS], "classes": list(CLASS_NAMES), "images": int(result["images"])}
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return path


def get_cli_parser():
    p = argparse.ArgumentParser(prog="python -m rsis_amd.cityscapes_eval", description="Cityscapes instance-level AP of a results folder")
    p.add_argument("--results", required=True, help="folder of the <sample>.txt files (mask paths relative to it)")
    p.add_argument("--gt", required=True, help="folder searched recursively for *_gtFine_instanceIds.png")
    p.add_argument("--json", default=None, help="write the result here")
    return p


def main(argv=None):
    a = get_cli_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rsis_amd.cityscapes_eval needs the GPU: the HIP library is the only compute path")
    res = evaluate_dirs(a.results, a.gt)
    sys.stdout.write(summary(res["averages"]))
    if a.json:
        print("%d images -> %s" % (res["images"], write_result_json(a.json, res)))
    return res


if __name__ == "__main__":
    main()
