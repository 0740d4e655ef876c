"""Reader of tests/golden/polymask.npz (written by tools/make_golden_polymask.py from the reference's own C mask API), and a float64
numpy statement of the rule the device kernel implements (rsis_amd/csrc/polymask.hip): a polygon's mask is the prefix parity, in
column-major element order, of the boundary positions its 5x-upsampled edge walk toggles.  The statement is written by hand from the
description of the algorithm; nothing of the reference is compiled or copied here."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polymask.npz")


def decode(counts, length):
    """run counts (starting with the run of zeros) -> (length,) uint8"""
    c = np.asarray(counts, np.int64)
    assert int(c.sum()) == length
    v = np.zeros((length,), np.uint8)
    pos = np.concatenate([[0], np.cumsum(c)])
    for j in range(1, len(c), 2):
        v[pos[j]:pos[j + 1]] = 1
    return v


def load():
    """-> {'records': [{'name', 'h', 'w', 'parts': [float64 (2k,) arrays], 'part_counts': [...], 'part_area': [...], 'counts', 'area'}],
    'urle': [{'name', 'h', 'w', 'counts', 'area', 'string'}], 'eval': {'images', 'gt_poly', 'gt_rle', 'dt', 'cats'}}"""
    z = np.load(PATH)
    names = json.loads(bytes(z["names"]).decode())
    xy, voff, poff = z["xy"], z["part_vertex_off"], z["rec_part_off"]
    pc, pco, rc, rco = z["part_counts"], z["part_counts_off"], z["rec_counts"], z["rec_counts_off"]
    recs = []
    for r, name in enumerate(names):
        ps = range(int(poff[r]), int(poff[r + 1]))
        recs.append({"name": name, "h": int(z["size"][r, 0]), "w": int(z["size"][r, 1]),
                     "parts": [xy[2 * int(voff[p]):2 * int(voff[p + 1])] for p in ps],
                     "part_counts": [pc[int(pco[p]):int(pco[p + 1])] for p in ps], "part_area": [int(z["part_area"][p]) for p in ps],
                     "counts": rc[int(rco[r]):int(rco[r + 1])], "area": int(z["rec_area"][r])})
    urle = []
    unames = json.loads(bytes(z["urle_names"]).decode())
    strings = json.loads(bytes(z["urle_strings"]).decode())
    for r, name in enumerate(unames):
        urle.append({"name": name, "h": int(z["urle_size"][r, 0]), "w": int(z["urle_size"][r, 1]),
                     "counts": z["urle_counts"][int(z["urle_off"][r]):int(z["urle_off"][r + 1])], "area": int(z["urle_area"][r]),
                     "string": strings[r]})
    ev = {k: json.loads(bytes(z["eval_" + k]).decode()) for k in ("images", "gt_poly", "gt_rle", "dt", "cats")}
    return {"records": recs, "urle": urle, "eval": ev}


def walk(xy):
    """xy: float64 (2k,) -> (u, v) int64: the points of the closed polygon's walk on the 5x grid, one per unit step of each edge's
    longer axis, both end points of every edge included"""
    p = np.asarray(xy, np.float64).reshape(-1, 2)
    x = (5.0 * p[:, 0] + .5).astype(np.int64)                       # (conversion truncates towards zero, as a C cast does)
    y = (5.0 * p[:, 1] + .5).astype(np.int64)
    k = len(x)
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = int(x[j]), int(x[(j + 1) % k]), int(y[j]), int(y[(j + 1) % k])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        d = np.arange(max(dx, dy) + 1, dtype=np.int64)
        if dx >= dy:
            t = dx - d if flip else d
            us.append(t + xs)
            if dx == 0:                                             # a zero-length edge: one point; its v is never used (same u as its neighbours)
                vs.append(np.zeros_like(t))
            else:
                s = np.float64(ye - ys) / np.float64(dx)
                vs.append(((np.float64(ys) + s * t.astype(np.float64)) + .5).astype(np.int64))
        else:
            t = dy - d if flip else d
            vs.append(t + ys)
            s = np.float64(xe - xs) / np.float64(dy)
            us.append(((np.float64(xs) + s * t.astype(np.float64)) + .5).astype(np.int64))
    return np.concatenate(us), np.concatenate(vs)


def toggles(xy, h, w):
    """-> (x, y) int64 of the boundary positions of one polygon part (y == h allowed: the first element of the next column)"""
    u, v = walk(xy)
    u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
    xd = np.where(u1 < u0, u1, u1 - 1).astype(np.float64)
    xd = (xd + .5) / 5.0 - .5
    ok = (u1 != u0) & (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.minimum(v1, v0).astype(np.float64)
    yd = (yd + .5) / 5.0 - .5
    yd = np.ceil(np.clip(yd, 0.0, float(h)))
    return xd[ok].astype(np.int64), yd[ok].astype(np.int64)


def part_mask(xy, h, w):
    """one polygon part -> (h * w,) uint8 in column-major element order: element p is set iff an odd number of positions are <= p"""
    x, y = toggles(xy, h, w)
    pos = x * h + y
    pos = pos[pos < h * w]
    t = np.bincount(pos, minlength=h * w) & 1
    return (np.cumsum(t) & 1).astype(np.uint8)


def record_mask(parts, h, w):
    """the union of the parts"""
    m = np.zeros((h * w,), np.uint8)
    for p in parts:
        m |= part_mask(p, h, w)
    return m
