"""The yardstick of the CVPPP tests: the measures of rsis_amd/cvppp_eval.py stated in float64 numpy from their definitions, loops over
labels, no cleverness (nothing here runs the challenge's Matlab scripts) -- and the reader of tests/golden/cvppp.npz, which
tools/make_golden_cvppp.py writes with these functions.

Every count is an integer and every score one fixed-order float64 expression of integers, so the device results are compared with
these for EQUALITY (counts array_equal, scores == with NaN positions equal)."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cvppp.npz")


def counts(a, g):
    """(256, 256) int64: [i, j] = number of pixels with a == i and g == j"""
    a, g = np.asarray(a), np.asarray(g)
    assert a.dtype == np.uint8 and g.dtype == np.uint8 and a.shape == g.shape
    t = np.zeros((256, 256), np.int64)
    np.add.at(t, (a.reshape(-1).astype(np.int64), g.reshape(-1).astype(np.int64)), 1)
    return t


def dice(o, n, m):
    """2 o / (n + m), one float64 division of two integers; 0 / 0 never wins a maximum: 0"""
    if n + m == 0:
        return 0.0
    return float(np.float64(2 * int(o)) / np.float64(int(n) + int(m)))


def best_dice(t):
    """BestDice(rows, columns) of a count table: every integer of the rows' range counts in the sum (ascending) and in the divisor"""
    n, m = t.sum(1), t.sum(0)
    ri, rj = np.nonzero(n)[0], np.nonzero(m)[0]
    lo_i, hi_i, lo_j, hi_j = int(ri[0]), int(ri[-1]), int(rj[0]), int(rj[-1])
    total = np.float64(0.0)
    for i in range(lo_i, hi_i + 1):
        best = 0.0
        for j in range(lo_j, hi_j + 1):
            d = dice(t[i, j], n[i], m[j])
            if best < d:
                best = d
        total = total + np.float64(best)
    return float(total / np.float64(hi_i - lo_i + 1))


def scores_from_counts(t):
    """the six scores of rsis_amd.cvppp_eval.SCORE_COLUMNS"""
    t = np.asarray(t, np.int64)
    n, m = t.sum(1), t.sum(0)
    ri, rj = np.nonzero(n)[0], np.nonzero(m)[0]
    lo_i, hi_i, lo_j, hi_j = int(ri[0]), int(ri[-1]), int(rj[0]), int(rj[-1])
    bd_in, bd_gt = best_dice(t), best_dice(t.T)
    npix = int(t.sum())
    f_in, f_gt = npix - int(n[lo_i]), npix - int(m[lo_j])
    both = int(t[lo_i + 1:, lo_j + 1:].sum())
    fgbg = float("nan") if f_in + f_gt == 0 else float(np.float64(2 * both) / np.float64(f_in + f_gt))
    diff = (hi_i - lo_i) - (hi_j - lo_j)
    return np.array([min(bd_in, bd_gt), fgbg, abs(diff), diff, bd_in, bd_gt], np.float64)


def nearest_resize(a, height, width):
    """the pixel-centre rule: src = min(floor((d + 0.5) * n_in / n_out), n_in - 1) per axis"""
    iy = [min(int(np.floor((d + 0.5) * a.shape[0] / height)), a.shape[0] - 1) for d in range(height)]
    ix = [min(int(np.floor((d + 0.5) * a.shape[1] / width)), a.shape[1] - 1) for d in range(width)]
    return a[np.array(iy)][:, np.array(ix)]


def scores(a, g):
    a, g = np.asarray(a), np.asarray(g)
    if a.shape != g.shape:
        a = nearest_resize(a, g.shape[0], g.shape[1])
    return scores_from_counts(counts(a, g))


def score_pairs(ins, gts):
    """drop-in for rsis_amd.cvppp_eval.score_pairs on the host"""
    return np.stack([scores(np.asarray(a), np.asarray(g)) for a, g in zip(ins, gts)]) if len(gts) else np.zeros((0, 6))


def same_scores(x, y):
    """bit-for-bit agreement of two score arrays: equal where numbers, NaN in the same places"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x.shape == y.shape and bool(np.array_equal(np.isnan(x), np.isnan(y))) and bool(np.all((x == y) | np.isnan(x)))


def load():
    """-> list of {name, in, gt, counts (sparse -> dense), scores}"""
    z = np.load(PATH)
    out = []
    for k, name in enumerate(bytes(z["names"]).decode().split("\n")):
        t = np.zeros((256 * 256,), np.int64)
        t[z["c%d_cell" % k]] = z["c%d_count" % k]
        out.append({"name": name, "in": z["c%d_in" % k], "gt": z["c%d_gt" % k], "counts": t.reshape(256, 256), "scores": z["c%d_scores" % k]})
    return out
