"""Writes tests/golden/cityscapes.npz: small Cityscapes-style cases (instance-id images, prediction masks, result lines) with what
tests/cityscapes_golden.py (the slow, direct statement of the measure) gives for them: per-image count tables, match lists, the 8 x 10
AP array and the averages.  Asserts that across the cases every branch of the definition fires at least once.

    python tools/make_golden_cityscapes.py          (CPU only; rewrites the fixture)

Layout: `ncases`; per case k `c{k}_n` images, `c{k}_aps`, `c{k}_all` = (allAp, allAp50%), `c{k}_cls` (8, 2) = (ap, ap50%) per class; per
image i of case k, prefix `c{k}_i{i}_`: gt (uint16), masks (P, h, w) uint8 DISTINCT masks, rows (Q,) = mask of every line, labels (Q,),
scores (Q,), counts (P + 1, S), ids (S,), rec_gt, rec_pred, rec_conf, rec_pairs (the arrays of cityscapes_eval.assign)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cityscapes_golden as G  # noqa: E402

ROAD = 7


def rect(shape, y0, y1, x0, x1):
    m = np.zeros(shape, np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def hand_case():
    """one 96 x 160 image in which every special rule is met on purpose, one 64 x 96 image with more of the same classes"""
    sh = (96, 160)
    gt = np.full(sh, ROAD, np.uint16)
    gt[10:40, 10:40] = 24001            # person, 900 pixels
    gt[50:58, 10:20] = 24002            # person, 80 pixels: below the minimum region size
    gt[60:80, 10:50] = 24               # a group of persons
    gt[10:50, 60:120] = 26001           # car
    gt[55:90, 60:100] = 26002           # car
    gt[0:8, 130:160] = 0                # void (unlabeled)
    gt[8:14, 130:160] = 4               # void (static)
    gt[60:90, 120:150] = 29001          # a caravan instance: raw value 29001 is not in the void list
    gt[42:48, 100:140] = 25001          # rider, 240 pixels, never predicted
    masks = [rect(sh, 10, 40, 10, 40), rect(sh, 10, 40, 12, 40), rect(sh, 11, 40, 10, 40), rect(sh, 50, 55, 10, 20),
             rect(sh, 62, 78, 12, 48), rect(sh, 0, 8, 130, 160), rect(sh, 85, 95, 5, 30), rect(sh, 10, 50, 70, 120),
             rect(sh, 55, 90, 95, 150), np.zeros(sh, np.uint8), rect(sh, 20, 30, 140, 155)]
    #        (mask, label, score): three persons on 24001 (a duplicate match, two tied scores), the small one, the group, void, road
    lines = [(0, 24, 0.9), (1, 24, 0.8), (2, 24, 0.8), (3, 24, 0.7), (4, 24, 0.6), (5, 24, 0.5), (6, 24, 0.4),
             (7, 26, 0.95), (8, 26, 0.3), (9, 26, 0.99), (10, 28, 0.5), (6, 7, 0.9), (8, 29, 0.9), (7, 27, 0.2), (7, 33, 0.2)]
    sh2 = (64, 96)
    gt2 = np.full(sh2, ROAD, np.uint16)
    gt2[5:30, 5:45] = 26003
    gt2[35:60, 5:30] = 24003
    gt2[35:60, 50:90] = 27001           # truck, predicted badly
    gt2[2:12, 60:80] = 33001            # bicycle
    masks2 = [rect(sh2, 5, 30, 5, 40), rect(sh2, 36, 60, 5, 30), rect(sh2, 30, 60, 40, 96), rect(sh2, 2, 12, 60, 80), rect(sh2, 0, 20, 55, 85)]
    lines2 = [(0, 26, 0.7), (1, 24, 0.8), (2, 27, 0.6), (3, 33, 0.9), (4, 33, 0.9), (0, 27, 0.1)]
    return [(gt, masks, lines), (gt2, masks2, lines2)]


def random_case(seed, n_images, shapes):
    r = np.random.default_rng(seed)
    out = []
    for i in range(n_images):
        sh = shapes[i % len(shapes)]
        gt = np.full(sh, ROAD, np.uint16)
        boxes = []
        for k in range(int(r.integers(3, 8))):
            h, w = int(r.integers(6, sh[0] // 2)), int(r.integers(6, sh[1] // 2))
            y0, x0 = int(r.integers(0, sh[0] - h)), int(r.integers(0, sh[1] - w))
            cls = int(r.choice([24, 26, 27, 33, 29, 0]))
            gt[y0:y0 + h, x0:x0 + w] = cls * 1000 + k + 1 if cls and r.random() < 0.85 else cls
            boxes.append((y0, y0 + h, x0, x0 + w, cls))
        masks, lines = [], []
        for (y0, y1, x0, x1, cls) in boxes:
            for _rep in range(int(r.integers(0, 3))):
                j = r.integers(-4, 5, 4)
                m = rect(sh, max(0, y0 + j[0]), min(sh[0], y1 + j[1]), max(0, x0 + j[2]), min(sh[1], x1 + j[3]))
                masks.append(m)
                for lab in {cls if cls in G.CLASSES else 24, int(r.choice([24, 26, 27, 33]))}:
                    lines.append((len(masks) - 1, lab, round(float(r.random()), 1)))
        out.append((gt, masks, lines))
    return out


CASES = [("hand", hand_case()), ("random small", random_case(11, 4, [(48, 64), (33, 77)])), ("random", random_case(12, 3, [(96, 160), (80, 100)]))]
NEEDED = ["duplicate match", "ignored through void alone", "ignored through group region alone", "ignored through small instance alone",
          "false positive kept", "ground truth, no prediction (AP 0)", "no ground truth (NaN)", "line of a non-evaluated class",
          "empty mask", "tied scores", "overlapping prediction masks", "29xxx instance under a prediction", "hard false negative",
          "true positive"]


def main():
    G.COUNTERS.clear()
    doc = {"ncases": np.int64(len(CASES))}
    for k, (name, images) in enumerate(CASES):
        res = G.evaluate([(gt, [(masks[m], lab, sc) for m, lab, sc in lines]) for gt, masks, lines in images])
        av = res["averages"]
        doc["c%d_n" % k] = np.int64(len(images))
        doc["c%d_aps" % k] = res["aps"]
        doc["c%d_all" % k] = np.array([av["allAp"], av["allAp50%"]])
        doc["c%d_cls" % k] = np.array([[av["classes"][n]["ap"], av["classes"][n]["ap50%"]] for n in G.NAMES])
        for i, ((gt, masks, lines), rec) in enumerate(zip(images, res["records"])):
            pre = "c%d_i%d_" % (k, i)
            counts, ids = G.direct_counts(gt, masks)
            doc[pre + "gt"] = gt
            doc[pre + "masks"] = np.stack(masks).astype(np.uint8) if masks else np.zeros((0,) + gt.shape, np.uint8)
            doc[pre + "rows"] = np.array([l[0] for l in lines], np.int64)
            doc[pre + "labels"] = np.array([l[1] for l in lines], np.int64)
            doc[pre + "scores"] = np.array([l[2] for l in lines], np.float64)
            doc[pre + "counts"], doc[pre + "ids"] = counts, ids
            for key in ("gt", "pred", "conf", "pairs"):
                doc[pre + "rec_" + key] = rec[key]
        print("case %d (%s): %d images, allAp %.6f, allAp50%% %.6f" % (k, name, len(images), av["allAp"], av["allAp50%"]))
    for key in sorted(G.COUNTERS):
        print("  %-45s %d" % (key, G.COUNTERS[key]))
    missing = [n for n in NEEDED if G.COUNTERS[n] < 1]
    assert not missing, "branches that never fired: %s" % missing
    out = os.path.join(ROOT, "tests", "golden", "cityscapes.npz")
    np.savez_compressed(out, **doc)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
