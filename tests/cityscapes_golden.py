"""The Cityscapes instance-level measure written the slow, direct way (the definition: docstring of rsis_amd/cityscapes_eval.py):
boolean images, np.count_nonzero(np.logical_and(gt == v, pred)) per pair, python loops and lists of dicts, no count table.  It shares
no code with the product module.  COUNTERS records how often each branch of the definition was taken (the fixture generator asserts that
every one fires)."""
import collections

import numpy as np

CLASSES = [24, 25, 26, 27, 28, 31, 32, 33]
NAMES = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
VOID = [0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30]
OVERLAPS = np.arange(0.5, 1.0, 0.05)
MIN_SIZE = 100

COUNTERS = collections.Counter()


def image_lists(gt, preds):
    """gt: (h, w) integer image of instance ids; preds: list of (mask (h, w), labelID, confidence) in line order.  Returns
    (gt_instances, pred_instances): lists of dicts in ascending instID / line order, each holding its matches."""
    gt = np.asarray(gt).astype(np.int64)
    void = np.isin(gt, VOID)
    gts = []
    for v in sorted(set(gt.reshape(-1).tolist())):
        label = v if v < 1000 else v // 1000
        if label in CLASSES:
            gts.append({"instID": v, "labelID": label, "pixelCount": int(np.count_nonzero(gt == v)), "matchedPred": []})
    out = []
    for line, (mask, label, conf) in enumerate(preds):
        if label not in CLASSES:
            COUNTERS["line of a non-evaluated class"] += 1
            continue
        m = np.asarray(mask) != 0
        if m.shape != gt.shape:
            raise ValueError("mask of size %s for a ground truth of %s" % (m.shape, gt.shape))
        area = int(np.count_nonzero(m))
        if area == 0:
            COUNTERS["empty mask"] += 1
            continue
        if np.count_nonzero(np.logical_and(gt // 1000 == 29, m)):
            COUNTERS["29xxx instance under a prediction"] += 1
        p = {"line": line, "labelID": label, "confidence": float(conf), "pixelCount": area,
             "voidIntersection": int(np.count_nonzero(np.logical_and(void, m))), "matchedGt": []}
        for g in gts:
            if g["labelID"] != label:
                continue
            inter = int(np.count_nonzero(np.logical_and(gt == g["instID"], m)))
            if inter > 0:
                g["matchedPred"].append({"pred": p, "intersection": inter})
                p["matchedGt"].append({"gt": g, "intersection": inter})
        out.append(p)
    for a in range(len(out)):
        for b in range(a + 1, len(out)):
            if np.count_nonzero(np.logical_and(np.asarray(preds[out[a]["line"]][0]) != 0, np.asarray(preds[out[b]["line"]][0]) != 0)):
                COUNTERS["overlapping prediction masks"] += 1
    return gts, out


def record(gts, preds):
    """the lists as the arrays rsis_amd.cityscapes_eval.assign returns (same layout, for comparison)"""
    gt = np.array([[g["instID"], g["labelID"], g["pixelCount"]] for g in gts], np.int64).reshape(-1, 3)
    pr = np.array([[p["line"], p["labelID"], p["pixelCount"], p["voidIntersection"]] for p in preds], np.int64).reshape(-1, 4)
    conf = np.array([p["confidence"] for p in preds], np.float64)
    pairs = []
    for k, p in enumerate(preds):
        for m in p["matchedGt"]:
            pairs.append((k, [g["instID"] for g in gts].index(m["gt"]["instID"]), m["intersection"]))
    return {"gt": gt, "pred": pr, "conf": conf, "pairs": np.array(pairs, np.int64).reshape(-1, 3)}


def lists_of(images, label, th):
    """(y_true list, y_score list, hard false negatives, haveGt, havePred) of one (class, threshold); images: list of (gts, preds)"""
    y_true, y_score, hard = [], [], 0
    have_gt = have_pred = False
    for gts, preds in images:
        cur_gt = [g for g in gts if g["labelID"] == label and g["instID"] >= 1000 and g["pixelCount"] >= MIN_SIZE]
        cur_pred = [p for p in preds if p["labelID"] == label]
        if cur_gt:
            have_gt = True
        if cur_pred:
            have_pred = True
        for g in cur_gt:
            found, score = False, -float("inf")
            for m in g["matchedPred"]:
                p = m["pred"]
                overlap = float(m["intersection"]) / float(g["pixelCount"] + p["pixelCount"] - m["intersection"])
                if overlap > th:
                    if found:
                        COUNTERS["duplicate match"] += 1
                        hi, lo = max(score, p["confidence"]), min(score, p["confidence"])
                        score = hi
                        y_true.append(0.0)
                        y_score.append(lo)
                    else:
                        found, score = True, p["confidence"]
            if not found:
                COUNTERS["hard false negative"] += 1
                hard += 1
                continue
            COUNTERS["true positive"] += 1
            y_true.append(1.0)
            y_score.append(score)
        for p in cur_pred:
            found = False
            for m in p["matchedGt"]:
                g = m["gt"]
                overlap = float(m["intersection"]) / float(g["pixelCount"] + p["pixelCount"] - m["intersection"])
                if overlap > th:
                    found = True
                    break
            if found:
                continue
            ignore = p["voidIntersection"]
            for m in p["matchedGt"]:
                g = m["gt"]
                if g["instID"] < 1000:
                    ignore += m["intersection"]
                if g["pixelCount"] < MIN_SIZE:      # (a group region below the size adds twice: two separate sums)
                    ignore += m["intersection"]
            if float(ignore) / float(p["pixelCount"]) <= th:
                COUNTERS["false positive kept"] += 1
                y_true.append(0.0)
                y_score.append(p["confidence"])
            else:
                why = []
                if p["voidIntersection"] > 0:
                    why.append("void")
                if any(m["gt"]["instID"] < 1000 for m in p["matchedGt"]):
                    why.append("group region")
                if any(m["gt"]["instID"] >= 1000 and m["gt"]["pixelCount"] < MIN_SIZE for m in p["matchedGt"]):
                    why.append("small instance")
                for w in why:
                    COUNTERS["ignored with " + w] += 1
                if len(why) == 1:
                    COUNTERS["ignored through " + why[0] + " alone"] += 1
    return y_true, y_score, hard, have_gt, have_pred


def ap_of(y_true, y_score, hard):
    """one operating point per distinct score, python loops"""
    order = sorted(range(len(y_score)), key=lambda i: y_score[i])
    ys = [y_score[i] for i in order]
    yt = [y_true[i] for i in order]
    n = len(ys)
    total = 0.0
    for t in yt:
        total += t
    if len(set(ys)) < n:
        COUNTERS["tied scores"] += 1
    precision, recall = [], []
    below = 0.0
    for k in range(n):
        if k == 0 or ys[k] != ys[k - 1]:
            tp = total - below
            fp = n - k - tp
            fn = below + hard
            precision.append(tp / (tp + fp))
            recall.append(tp / (tp + fn))
        below += yt[k]
    precision.append(1.0)
    recall.append(0.0)
    rc = [recall[0]] + recall + [0.0]
    ap = 0.0
    for i in range(len(precision)):
        ap += precision[i] * (-0.5 * rc[i + 2] + 0.0 * rc[i + 1] + 0.5 * rc[i])
    return ap


def evaluate(images):
    """images: list of (gt image, preds) -> {"aps": (8, 10), "records": per-image arrays, "averages": dict}"""
    lists = [image_lists(gt, preds) for gt, preds in images]
    aps = np.zeros((len(CLASSES), len(OVERLAPS)))
    for ci, label in enumerate(CLASSES):
        for ti, th in enumerate(OVERLAPS):
            y_true, y_score, hard, have_gt, have_pred = lists_of(lists, label, th)
            if have_gt and have_pred:
                if y_true:
                    aps[ci, ti] = ap_of(y_true, y_score, hard)
                else:                       # no operating point: precision [1], recall [0] -> 0
                    COUNTERS["ground truth and predictions, empty lists"] += 1
                    aps[ci, ti] = 0.0
            elif have_gt:
                COUNTERS["ground truth, no prediction (AP 0)"] += 1
                aps[ci, ti] = 0.0
            else:
                COUNTERS["no ground truth (NaN)"] += 1
                aps[ci, ti] = float("nan")
    return {"aps": aps, "records": [record(g, p) for g, p in lists], "averages": averages(aps)}


def averages(aps):
    def mean_of(vals):
        vals = [v for v in vals if v == v]
        return sum(vals) / len(vals) if vals else float("nan")
    aps = np.asarray(aps)
    out = {"allAp": mean_of([float(v) for v in aps.reshape(-1)]), "allAp50%": mean_of([float(v) for v in aps[:, 0]]), "classes": {}}
    for ci, name in enumerate(NAMES):
        row = [float(v) for v in aps[ci]]
        out["classes"][name] = {"ap": sum(row) / len(row), "ap50%": row[0]}
    return out


def direct_counts(gt, masks):
    """(P + 1, S) int64 table and the sorted ids, by boolean images (the reference for the kernel on small cases)"""
    gt = np.asarray(gt).astype(np.int64)
    ids = np.array(sorted(set(gt.reshape(-1).tolist())), np.int64)
    out = np.zeros((len(masks) + 1, len(ids)), np.int64)
    for s, v in enumerate(ids):
        here = gt == v
        for p, m in enumerate(masks):
            out[p, s] = np.count_nonzero(np.logical_and(here, np.asarray(m) != 0))
        out[len(masks), s] = np.count_nonzero(here)
    return out, ids
