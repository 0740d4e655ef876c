"""Reader of tests/golden/cocoeval.npz (written by tools/make_golden_cocoeval.py from the reference's own COCOeval)."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cocoeval.npz")
T = 10


def load():
    z = np.load(PATH)
    sets = []
    for s in range(int(z["nsets"])):
        sets.append({"gt": json.loads(bytes(z["set%d_gt" % s]).decode()), "dt": json.loads(bytes(z["set%d_dt" % s]).decode()),
                     "cats": [int(c) for c in z["set%d_cats" % s]]})
    runs = []
    for n, row in enumerate(z["runs"]):
        g = lambda k: z["run%d_%s" % (n, k)]
        S = sets[int(row[0])]
        imgs = sorted(set(r["image_id"] for r in S["gt"] + S["dt"]))
        cells, o = [], {k: 0 for k in ("dtm", "gtm", "dtig", "gtig", "dtids", "gtids", "dtscores")}

        def take(k, n_):
            v = g(k)[o[k]:o[k] + n_]
            o[k] += n_
            return v
        for D, G in g("cell_dims"):
            if D < 0:
                cells.append(None)
                continue
            D, G = int(D), int(G)
            cells.append({"dtMatches": take("dtm", T * D).reshape(T, D), "gtMatches": take("gtm", T * G).reshape(T, G),
                          "dtIgnore": take("dtig", T * D).reshape(T, D), "gtIgnore": take("gtig", G), "dtIds": take("dtids", D),
                          "gtIds": take("gtids", G), "dtScores": take("dtscores", D)})
        ious, oi = [], 0
        for d_, g_ in g("iou_shape"):
            ious.append(g("ious")[oi:oi + d_ * g_].reshape(int(d_), int(g_)))
            oi += int(d_ * g_)
        runs.append({"set": int(row[0]), "useCats": int(row[1]), "maxDets": [int(v) for v in row[2:5]], "imgIds": imgs, "catIds": S["cats"],
                     "cells": cells, "ious": ious, "precision": g("precision"), "recall": g("recall"), "stats": g("stats"),
                     "summary": bytes(g("summary")).decode().splitlines()})
    return sets, runs


def per_k_from_cells(run, A=4):
    """the golden per-cell matches in the form rsis_amd.cocoeval.accumulate_cells takes"""
    I = len(run["imgIds"])
    K = len(run["catIds"]) if run["useCats"] else 1
    out = []
    for k in range(K):
        ck = {"cells": False, "dtm": [], "dti": [], "gig": []}
        for a in range(A):
            E = [e for e in run["cells"][(k * A + a) * I:(k * A + a + 1) * I] if e is not None]
            ck["cells"] = ck["cells"] or bool(E)
            cat = lambda key, ax, empty: np.concatenate([e[key] for e in E], axis=ax) if E else empty
            ck["dtm"].append(cat("dtMatches", 1, np.zeros((T, 0), np.int64)).T)
            ck["dti"].append(cat("dtIgnore", 1, np.zeros((T, 0), np.int64)).T)
            ck["gig"].append(cat("gtIgnore", 0, np.zeros((0,), np.int64)))
            if a == 0:
                ck["scores"] = cat("dtScores", 0, np.zeros((0,)))
                ck["rank"] = np.concatenate([np.arange(len(e["dtIds"])) for e in E]) if E else np.zeros((0,), np.int64)
        out.append(ck)
    return out
