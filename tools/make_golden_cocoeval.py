"""Writes tests/golden/cocoeval.npz: small COCO 'segm' evaluation cases and what the REFERENCE's own (modified) pycocotools COCOeval
computes for them -- every cell's ious / dtMatches / gtMatches / dtIgnore / gtIgnore, and precision, recall, stats.

    make -C oracle && python tools/make_golden_cocoeval.py [--ref <reference checkout>]

The reference's cocoeval.py is IMPORTED at run time from the checkout (nothing of it is copied here).  Three provisions make it run
under Python 3 without its Cython extension: `pycocotools._mask` is a ctypes shim over oracle/_ref/libmaskapi_ref.so (the
reference's unmodified maskApi.c, built by oracle/Makefile); np.linspace accepts the float `num` the file passes and np.float
exists; a small stand-in replaces its COCO class.  Each case the tests rely on is asserted below, so that a regenerated fixture
cannot silently lose it."""
import argparse
import copy
import ctypes
import io
import json
import os
import sys
import types
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import maskapi_ref  # noqa: E402


class _RLE(ctypes.Structure):
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def _mask_shim():
    L = ctypes.CDLL(maskapi_ref._PATH)
    L.rleFrString.argtypes = [ctypes.POINTER(_RLE), ctypes.c_char_p, ctypes.c_ulong, ctypes.c_ulong]
    L.rleFrString.restype = None
    L.rleIou.argtypes = [ctypes.POINTER(_RLE), ctypes.POINTER(_RLE), ctypes.c_ulong, ctypes.c_ulong, ctypes.c_void_p, ctypes.c_void_p]
    L.rleIou.restype = None
    L.rleArea.argtypes = [ctypes.POINTER(_RLE), ctypes.c_ulong, ctypes.c_void_p]
    L.rleArea.restype = None
    L.rleFree.argtypes = [ctypes.POINTER(_RLE)]
    L.rleFree.restype = None

    def fr(objs):
        R = (_RLE * len(objs))()
        for i, o in enumerate(objs):
            c = o["counts"] if isinstance(o["counts"], bytes) else o["counts"].encode("ascii")
            L.rleFrString(ctypes.byref(R[i]), c, o["size"][0], o["size"][1])
        return R

    def free(R):
        for i in range(len(R)):
            L.rleFree(ctypes.byref(R[i]))

    def iou(dt, gt, pyiscrowd):
        m, n = len(dt), len(gt)
        if m == 0 or n == 0:
            return []
        crowd = np.array(pyiscrowd, dtype=np.uint8)
        D, G = fr(dt), fr(gt)
        out = np.zeros((m * n,), np.float64)
        L.rleIou(D, G, m, n, crowd.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
        free(D)
        free(G)
        return out.reshape((m, n), order="F")

    def area(objs):
        R = fr(objs)
        a = np.zeros((len(objs),), np.uint32)
        L.rleArea(R, len(objs), a.ctypes.data_as(ctypes.c_void_p))
        free(R)
        return a

    mod = types.ModuleType("pycocotools._mask")
    mod.iou, mod.area = iou, area
    mod.merge = mod.frPyObjects = mod.encode = mod.decode = mod.toBbox = None
    return mod


def import_reference_cocoeval(ref):
    sys.modules["pycocotools._mask"] = _mask_shim()
    sys.path.insert(0, os.path.join(ref, "src", "coco", "PythonAPI"))
    _ls = np.linspace
    np.linspace = lambda a, b, num=50, **kw: _ls(a, b, int(num), **kw)
    np.float = float
    from pycocotools.cocoeval import COCOeval
    from pycocotools import mask as maskUtils
    return COCOeval, maskUtils


class StandInCOCO(object):
    """what COCOeval needs of the reference's COCO class"""

    def __init__(self, anns):
        self.anns = {a["id"]: a for a in anns}

    def getAnnIds(self, imgIds=[], catIds=[]):
        return [a["id"] for a in self.anns.values() if (not len(imgIds) or a["image_id"] in imgIds) and (not len(catIds) or a["category_id"] in catIds)]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def getImgIds(self):
        return sorted(set(a["image_id"] for a in self.anns.values()))

    def getCatIds(self):
        return sorted(set(a["category_id"] for a in self.anns.values()))

    def annToRLE(self, ann):
        return ann["segmentation"]


def seg(mask):
    _c, s = maskapi_ref.encode(mask)
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": s.decode("ascii")}


def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def blob(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0, h), rng.uniform(0, w)
    ry, rx = rng.uniform(0.08, 0.35) * h, rng.uniform(0.08, 0.35) * w
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1).astype(np.uint8)


def set_mixed(rng):
    """hand-made traps: three sizes, ignore, crowd matched twice, score ties, equal IoUs, empty cells and an empty mask"""
    gt, dt = [], []
    g = lambda img, cat, m, **kw: gt.append(dict(image_id=img, category_id=cat, segmentation=seg(m), **kw))
    d = lambda img, cat, m, score: dt.append(dict(image_id=img, category_id=cat, segmentation=seg(m), score=score))
    H, W = 200, 264
    small, medium, large = rect(H, W, 5, 25, 5, 25), rect(H, W, 40, 90, 10, 60), rect(H, W, 60, 170, 120, 230)
    g("img_a", 1, small)
    g("img_a", 1, medium)
    g("img_a", 2, large)
    crowd = rect(H, W, 0, 60, 100, 200)
    g("img_a", 3, crowd, iscrowd=1)
    g("img_a", 3, rect(H, W, 100, 140, 10, 50), ignore=1)
    g("img_a", 3, rect(H, W, 150, 190, 10, 50))
    d("img_a", 1, rect(H, W, 5, 25, 6, 26), 0.9)
    d("img_a", 1, rect(H, W, 42, 92, 10, 60), 0.8)
    d("img_a", 1, rect(H, W, 40, 90, 12, 62), 0.8)                  # exact tie in the category, same target
    d("img_a", 1, rect(H, W, 0, 0, 0, 0), 0.7)                      # an empty mask
    d("img_a", 2, rect(H, W, 62, 170, 120, 228), 0.95)
    d("img_a", 2, rect(H, W, 60, 100, 120, 160), 0.5)
    d("img_a", 3, rect(H, W, 5, 30, 105, 140), 0.6)                 # two detections inside the crowd region
    d("img_a", 3, rect(H, W, 30, 55, 150, 190), 0.55)
    d("img_a", 3, rect(H, W, 100, 140, 10, 50), 0.5)                # on the ignored ground truth
    d("img_a", 3, rect(H, W, 152, 190, 10, 50), 0.45)
    d("img_a", 5, rect(H, W, 10, 50, 10, 50), 0.4)                  # category 5 has no ground truth anywhere
    h, w = 37, 53
    g("img_b", 1, rect(h, w, 5, 25, 0, 10))                         # two ground truths, the same IoU (9 / 11) to one detection
    g("img_b", 1, rect(h, w, 5, 25, 2, 12))
    d("img_b", 1, rect(h, w, 5, 25, 1, 11), 0.9)
    d("img_b", 1, rect(h, w, 5, 25, 0, 10), 0.9)
    d("img_b", 2, rect(h, w, 0, 10, 20, 40), 0.3)
    g("img_b", 4, rect(h, w, 26, 36, 30, 50), iscrowd=1, ignore=1)
    d("img_b", 4, rect(h, w, 27, 35, 31, 45), 0.8)
    d("img_b", 4, rect(h, w, 27, 35, 40, 50), 0.8)
    for j in range(3):                                               # detections, no ground truth
        d("img_c", 1 + j, blob(rng, 64, 48), round(float(rng.uniform()), 2))
    g("img_d", 2, blob(rng, 100, 132))                               # ground truth, no detection
    g("img_d", 4, blob(rng, 100, 132))
    return gt, dt, list(range(1, 6))


def set_evalshape(rng):
    """the shape eval.py emits: every predicted mask once per category with different scores, 10 masks x 20 categories per image"""
    gt, dt = [], []
    for img, (h, w) in (("synthetic_000000", (64, 64)), ("synthetic_000001", (96, 80)), ("synthetic_000002", (200, 264))):
        truth = [blob(rng, h, w) for _ in range(3)]
        for m in truth:
            gt.append(dict(image_id=img, category_id=int(rng.integers(1, 21)), segmentation=seg(m)))
        for j in range(10):
            m = truth[j % 3].copy() if j < 6 else blob(rng, h, w)
            if j < 6:                                                # a perturbed copy of a ground truth
                m = np.roll(m, int(rng.integers(-4, 5)), axis=int(rng.integers(0, 2)))
            s = seg(m)
            obj = float(rng.uniform(0.5, 1.0))
            probs = rng.dirichlet(np.ones(21) * 0.3)
            for c in range(1, 21):
                dt.append(dict(image_id=img, category_id=c, segmentation=s, score=float(np.float32(probs[c])) * obj))
    return gt, dt, list(range(1, 21))


def finish(gt, dt, maskUtils):
    """what the reference's loadRes adds: ids, areas, iscrowd"""
    for i, a in enumerate(gt):
        a.setdefault("id", i + 1)
        a.setdefault("iscrowd", 0)
        a.setdefault("area", float(maskUtils.area(a["segmentation"])))
    for i, a in enumerate(dt):
        a["id"] = i + 1
        a["iscrowd"] = 0
        a["area"] = float(maskUtils.area(a["segmentation"]))


def run_reference(COCOeval, gt, dt, img_ids, cat_ids, use_cats, max_dets):
    E = COCOeval(StandInCOCO(copy.deepcopy(gt)), StandInCOCO(copy.deepcopy(dt)), "segm")
    E.params.maxDets = list(max_dets)
    E.params.useCats = use_cats
    E.params.imgIds = sorted(img_ids)
    E.params.catIds = list(cat_ids)
    text = io.StringIO()
    with redirect_stdout(text):
        E.evaluate()
        ious = dict(E.ious)
        E.accumulate()
        E.summarize()
    return E, ious, text.getvalue()


def pack_run(prefix, E, ious, text, out):
    p = E.params
    shapes, flat = [], []
    for i in E._paramsEval.imgIds:
        for c in (E._paramsEval.catIds if p.useCats else [-1]):
            m = np.asarray(ious[i, c], np.float64)
            shapes.append(m.shape if m.ndim == 2 else (0, 0))
            flat.append(m.reshape(-1))
    out[prefix + "iou_shape"] = np.array(shapes, np.int64).reshape(-1, 2)
    out[prefix + "ious"] = np.concatenate(flat) if flat else np.zeros((0,))
    dims, cat = [], {k: [] for k in ("dtm", "gtm", "dtig", "gtig", "dtids", "gtids", "dtscores")}
    for e in E.evalImgs:
        if e is None:
            dims.append((-1, -1))
            continue
        dims.append((len(e["dtIds"]), len(e["gtIds"])))
        cat["dtm"].append(np.asarray(e["dtMatches"], np.int64).reshape(-1))
        cat["gtm"].append(np.asarray(e["gtMatches"], np.int64).reshape(-1))
        cat["dtig"].append(np.asarray(e["dtIgnore"], np.int64).reshape(-1))
        cat["gtig"].append(np.asarray(e["gtIgnore"], np.int64).reshape(-1))
        cat["dtids"].append(np.asarray(e["dtIds"], np.int64))
        cat["gtids"].append(np.asarray(e["gtIds"], np.int64))
        cat["dtscores"].append(np.asarray(e["dtScores"], np.float64))
    out[prefix + "cell_dims"] = np.array(dims, np.int64)
    for k, v in cat.items():
        out[prefix + k] = np.concatenate(v) if v else np.zeros((0,), np.float64 if k == "dtscores" else np.int64)
    out[prefix + "precision"] = np.asarray(E.eval["precision"], np.float64)
    out[prefix + "recall"] = np.asarray(E.eval["recall"], np.float64)
    out[prefix + "stats"] = np.asarray(E.stats, np.float64)
    out[prefix + "summary"] = np.frombuffer("\n".join(l for l in text.splitlines() if l.startswith(" Average")).encode(), np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cocoeval.npz"))
    a = ap.parse_args()
    assert maskapi_ref.available(), "run `make -C oracle` first"
    COCOeval, maskUtils = import_reference_cocoeval(a.ref)
    rng = np.random.default_rng(20240611)
    sets = [set_mixed(rng), set_evalshape(rng)]
    out = {"nsets": np.int64(len(sets))}
    for s, (gt, dt, cats) in enumerate(sets):
        finish(gt, dt, maskUtils)
        out["set%d_gt" % s] = np.frombuffer(json.dumps(gt).encode(), np.uint8)
        out["set%d_dt" % s] = np.frombuffer(json.dumps(dt).encode(), np.uint8)
        out["set%d_cats" % s] = np.array(cats, np.int64)
    runs = [(0, 1, [1, 10, 100]), (0, 0, [1, 100, 100]), (1, 0, [1, 100, 100]), (1, 1, [1, 10, 100]), (1, 1, [1, 100, 100])]
    out["runs"] = np.array([(s, u) + tuple(m) for s, u, m in runs], np.int64)
    kept = []
    for n, (s, use_cats, max_dets) in enumerate(runs):
        gt, dt, cats = sets[s]
        imgs = sorted(set(r["image_id"] for r in gt + dt))
        E, ious, text = run_reference(COCOeval, gt, dt, imgs, cats, use_cats, max_dets)
        pack_run("run%d_" % n, E, ious, text, out)
        kept.append((E, ious))
        print("run %d (set %d, useCats %d, maxDets %s): stats %s" % (n, s, use_cats, max_dets, np.array2string(np.asarray(E.stats), precision=4)))

    # ---- the cases the tests rely on ----
    gt0, dt0, _ = sets[0]
    sizes = set(tuple(r["segmentation"]["size"]) for r in gt0 + dt0)
    assert len(sizes) >= 3 and any(h >= 200 and w >= 264 for h, w in sizes)
    areas = [r["area"] for r in gt0 if r["image_id"] == "img_a"]
    assert any(v < 32 ** 2 for v in areas) and any(32 ** 2 < v < 96 ** 2 for v in areas) and any(v > 96 ** 2 for v in areas)
    assert any(r.get("ignore") for r in gt0) and any(r["iscrowd"] for r in gt0)
    assert any(r["area"] == 0 for r in dt0), "an empty mask"
    E0, ious0 = kept[0]
    crowd_ids = set(r["id"] for r in gt0 if r["iscrowd"])
    twice = False
    for e in E0.evalImgs:
        if e is not None and e["aRng"][1] == 1e5 ** 2 and e["aRng"][0] == 0:
            row = [int(v) for v in e["dtMatches"][0] if v > 0]
            twice = twice or any(row.count(c) >= 2 for c in crowd_ids)
    assert twice, "one crowd region matched by two detections"
    keys = {}
    for r in dt0:
        keys.setdefault((r["image_id"], r["category_id"], r["score"]), []).append(r)
    assert any(len(v) > 1 for v in keys.values()), "exact score ties inside a category"
    m = np.asarray(ious0["img_b", 1])
    assert any(m[i, 0] == m[i, 1] and m[i, 0] >= 0.5 for i in range(m.shape[0])), "two ground truths with the same IoU to one detection"
    assert np.asarray(ious0["img_c", 1]).size == 0
    assert not any(r["image_id"] == "img_c" for r in gt0) and any(r["image_id"] == "img_c" for r in dt0)
    assert not any(r["image_id"] == "img_d" for r in dt0) and any(r["image_id"] == "img_d" for r in gt0)
    assert not any(r["category_id"] == 5 for r in gt0) and (E0.eval["precision"][:, :, 4] == -1).all()
    gt1, dt1, _ = sets[1]
    per = {}
    for r in dt1:
        per[r["image_id"]] = per.get(r["image_id"], 0) + 1
    assert all(v == 200 for v in per.values())
    E2 = kept[2][0]
    assert all(len(e["dtIds"]) == 100 for e in E2.evalImgs if e is not None), "maxDets truncates 200 detections to 100"
    assert list(E2.params.maxDets) == [1, 100, 100]
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
