"""Wall time of the COCO segm evaluation on a Pascal-val-sized synthetic workload (NOTES.md): 1449 images of 375 x 500, 10 predicted
masks x 20 classes each (every mask once per class, as rsis_amd.eval emits them), about 3 ground truths per image.

    python tools/bench_cocoeval.py [--images 1449]            # device: evaluate() + accumulate(), and the grouped intersection launch
    python tools/bench_cocoeval.py --reference --images 200   # the reference's COCOeval on the same records (host, needs the checkout)

The two modes build the same records from the same seed.  The intersection launch is timed alone with device events over repeated
launches; its bytes are what the kernel reads: every detection row once per ground-truth tile, every ground-truth row once per
detection tile (tiles of 8 x 4, rsis_amd/csrc/maskeval.hip)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, NMASK, NCLS = 375, 500, 10, 21


def image_boxes(rng):
    """3 ground-truth boxes + 10 predicted boxes (6 jittered ground truths, 4 random), scores [10][20], ground-truth classes [3]"""
    def box():
        h, w = int(rng.integers(30, 200)), int(rng.integers(30, 260))
        y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        return y, y + h, x, x + w
    gt = [box() for _ in range(3)]
    dt = []
    for j in range(NMASK):
        if j < 6:
            y0, y1, x0, x1 = gt[j % 3]
            dy, dx = int(rng.integers(-12, 13)), int(rng.integers(-12, 13))
            dt.append((max(0, y0 + dy), min(H, y1 + dy), max(0, x0 + dx), min(W, x1 + dx)))
        else:
            dt.append(box())
    scores = rng.dirichlet(np.ones(NCLS) * 0.3, size=NMASK)[:, 1:] * rng.uniform(0.5, 1.0, size=(NMASK, 1))
    return gt, dt, scores, [int(c) for c in rng.integers(1, NCLS, size=3)]


def rasterise(boxes):
    m = np.zeros((len(boxes), W, H), np.uint8)                     # column-major element order (x, y)
    for k, (y0, y1, x0, x1) in enumerate(boxes):
        m[k, x0:x1, y0:y1] = 1
    return m.reshape(len(boxes), -1)


def device(n_images):
    import torch
    from rsis_amd import cocoeval as CE
    rng = np.random.default_rng(7)
    ev = CE.COCOEvalDevice()
    ev.keep_intersect_inputs = True
    ids = ["img_%06d" % i for i in range(n_images)]
    for i in ids:
        gt, dt, scores, gcls = image_boxes(rng)
        ev.add_gt_masks(i, torch.from_numpy(rasterise(gt)).cuda(), gcls)
        rows = [j for j in range(NMASK) for _c in range(1, NCLS)]
        ev.add_dt_masks(i, torch.from_numpy(rasterise(dt)).cuda(), [c for _j in range(NMASK) for c in range(1, NCLS)],
                        scores.reshape(-1).tolist(), rows=rows)
    out = {"images": n_images, "records": n_images * NMASK * (NCLS - 1)}
    for use_cats in (1, 0):
        ev.params.maxDets, ev.params.useCats = [1, 100, 100], use_cats
        ev.params.imgIds, ev.params.catIds = ids, list(range(1, NCLS))
        for rep in range(3):                                        # the first pass loads the code objects
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ev.accumulate()
            t2 = time.perf_counter()
        ev.summarize()
        out["useCats%d" % use_cats] = {"evaluate_s": t1 - t0, "accumulate_s": t2 - t1, "stats": [float(v) for v in ev.stats]}
    pool, jd, njobs, nblk, ooff = ev._res["intersect_inputs"]
    inter = torch.empty((ooff,), dtype=torch.int32, device="cuda")
    L = CE.lib()
    jobs = jd.cpu().numpy()
    nbytes = int(sum(8 * j[4] * (j[2] * -(-j[3] // 4) + j[3] * -(-j[2] // 8)) for j in jobs))
    reps = 50
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        CE.check(L.rsis_mask_intersect_batch(CE.ptr(pool), pool.numel(), CE.ptr(jd), njobs, nblk, CE.ptr(inter), ooff, CE.stream()), "intersect")
    e0.record()
    for _ in range(reps):
        CE.check(L.rsis_mask_intersect_batch(CE.ptr(pool), pool.numel(), CE.ptr(jd), njobs, nblk, CE.ptr(inter), ooff, CE.stream()), "intersect")
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    out["intersect"] = {"jobs": njobs, "blocks": nblk, "pool_bytes": pool.numel() * 8, "bytes_read": nbytes, "ms_per_launch": ms,
                        "GB_per_s": nbytes / ms / 1e6, "note": "includes the zero-fill of the output; the pool fits the 256 MiB cache "
                        "only in part"}
    print(json.dumps(out))


def reference(n_images, ref):
    from oracle import maskapi_ref
    from tools import make_golden_cocoeval as G
    COCOeval, maskUtils = G.import_reference_cocoeval(ref)
    rng = np.random.default_rng(7)
    gts, dts, ids = [], [], ["img_%06d" % i for i in range(n_images)]
    for i in ids:
        gt, dt, scores, gcls = image_boxes(rng)
        for b, c in zip(gt, gcls):
            gts.append(dict(image_id=i, category_id=c, segmentation=G.seg(G.rect(H, W, *b))))
        for j, b in enumerate(dt):
            s = G.seg(G.rect(H, W, *b))
            for c in range(1, NCLS):
                dts.append(dict(image_id=i, category_id=c, segmentation=s, score=float(scores[j, c - 1])))
    G.finish(gts, dts, maskUtils)
    out = {"images": n_images, "records": len(dts), "host": "reference COCOeval, Python 3 + ctypes over its maskApi.c, one CPU core"}
    for use_cats in (1, 0):
        t0 = time.perf_counter()
        E, _ious, _text = G.run_reference(COCOeval, gts, dts, ids, list(range(1, NCLS)), use_cats, [1, 100, 100])
        out["useCats%d" % use_cats] = {"evaluate_accumulate_summarize_s": time.perf_counter() - t0, "stats": [float(v) for v in E.stats]}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1449)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    a = ap.parse_args()
    reference(a.images, a.ref) if a.reference else device(a.images)
