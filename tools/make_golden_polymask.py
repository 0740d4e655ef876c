"""Writes tests/golden/polymask.npz: polygon and uncompressed-RLE segmentations and what the REFERENCE's own C mask API makes of them
-- the run counts of rleFrPoly for every polygon part, of rleMerge (intersect = 0) for every record, and their areas -- plus a small
synthetic evaluation whose ground truth is given twice: as polygons / uncompressed counts, and converted by that library to
compressed RLE.

    make -C oracle && python tools/make_golden_polymask.py

oracle/_ref/libmaskapi_ref.so is the reference's unmodified maskApi.c (built by oracle/Makefile); its functions are bound with ctypes
right here, nothing of it is copied.  Each case the tests rely on is asserted below, so that a regenerated fixture cannot silently
lose it."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import maskapi_ref  # noqa: E402
import polymask_golden as PG  # noqa: E402  (the tests' numpy statement: used here only to ASSERT that a named case is present)


class _RLE(ctypes.Structure):
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def _bind():
    L = ctypes.CDLL(maskapi_ref._PATH)
    P = ctypes.POINTER(_RLE)
    L.rleFrPoly.argtypes = [P, ctypes.c_void_p, ctypes.c_ulong, ctypes.c_ulong, ctypes.c_ulong]
    L.rleFrPoly.restype = None
    L.rleMerge.argtypes = [P, P, ctypes.c_ulong, ctypes.c_int]
    L.rleMerge.restype = None
    L.rleFrString.argtypes = [P, ctypes.c_char_p, ctypes.c_ulong, ctypes.c_ulong]
    L.rleFrString.restype = None
    L.rleArea.argtypes = [P, ctypes.c_ulong, ctypes.c_void_p]
    L.rleArea.restype = None
    L.rleToString.argtypes = [P]
    L.rleToString.restype = ctypes.c_void_p
    L.rleFree.argtypes = [P]
    L.rleFree.restype = None
    return L


L = None


def _counts(R):
    return np.ctypeslib.as_array(R.cnts, shape=(R.m,)).astype(np.uint32).copy() if R.m else np.zeros((0,), np.uint32)


def _area(R):
    a = np.zeros((1,), np.uint32)
    L.rleArea(ctypes.byref(R), 1, a.ctypes.data_as(ctypes.c_void_p))
    return int(a[0])


def _string(R):
    sp = L.rleToString(ctypes.byref(R))
    s = ctypes.string_at(sp)
    ctypes.CDLL(None).free(ctypes.c_void_p(sp))
    return s


def ref_record(parts, h, w):
    """-> ([counts of each part], [area of each part], counts of the merged record, its area, its compressed string)"""
    R = (_RLE * len(parts))()
    pc, pa = [], []
    for i, p in enumerate(parts):
        xy = np.ascontiguousarray(p, np.float64)
        L.rleFrPoly(ctypes.byref(R[i]), xy.ctypes.data_as(ctypes.c_void_p), len(xy) // 2, h, w)
        pc.append(_counts(R[i]))
        pa.append(_area(R[i]))
    M = _RLE()
    L.rleMerge(R, ctypes.byref(M), len(parts), 0)
    mc, ma, ms = _counts(M), _area(M), _string(M)
    back = _RLE()                                                   # the text form decodes to the same counts
    L.rleFrString(ctypes.byref(back), ms, h, w)
    assert np.array_equal(_counts(back), mc)
    for i in range(len(parts)):
        L.rleFree(ctypes.byref(R[i]))
    L.rleFree(ctypes.byref(M))
    L.rleFree(ctypes.byref(back))
    return pc, pa, mc, ma, ms


def ref_from_counts(counts, h, w):
    """uncompressed counts -> (area, compressed string), through the reference's rleArea / rleToString"""
    c = np.ascontiguousarray(counts, np.uint32)
    R = _RLE(h, w, len(c), c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))
    return _area(R), _string(R)


def regular(cx, cy, r, n, phase=0.0):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1).reshape(-1)


def star(cx, cy, r0, r1, n):
    a = 2 * np.pi * np.arange(2 * n) / (2 * n) + 0.1
    r = np.where(np.arange(2 * n) % 2 == 0, r1, r0)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1).reshape(-1)


def named_cases():
    f = lambda *v: np.array(v, np.float64)
    C = []
    add = lambda name, h, w, *parts: C.append((name, h, w, [np.asarray(p, np.float64) for p in parts]))
    add("size_13x11", 13, 11, f(1.5, 2.0, 9.5, 1.5, 10.0, 11.5, 4.0, 12.5, 0.5, 7.0))
    add("size_300x7", 300, 7, f(0.5, 10.0, 6.5, 40.5, 5.0, 290.0, 1.0, 250.5))
    add("one_word_column", 64, 3, f(0.0, 5.0, 3.0, 20.0, 2.5, 60.0, 0.5, 63.5))
    add("h_is_1", 1, 40, f(3.0, 0.0, 30.5, 0.0, 30.5, 1.0, 3.0, 1.0))
    add("w_is_1", 50, 1, f(0.0, 4.5, 1.0, 10.0, 1.0, 40.0, 0.0, 44.5))
    add("outside_every_side", 20, 30, f(-5.0, 10.0, 15.0, -6.0, 36.0, 10.0, 15.0, 27.0))
    add("clamped_to_h_mid_column", 24, 20, f(5.0, 10.0, 12.0, 10.0, 12.0, 30.0, 5.0, 30.0))
    add("position_hw_dropped", 24, 20, f(15.0, 5.0, 24.0, 5.0, 24.0, 29.0, 15.0, 29.0))
    add("entirely_outside", 24, 20, f(25.0, 3.0, 40.0, 3.0, 33.0, 20.0))
    add("repeated_consecutive_vertex", 32, 32, f(4.0, 4.0, 20.0, 6.0, 20.0, 6.0, 24.0, 25.0, 6.0, 22.0))
    add("repeated_first_last_vertex", 32, 32, f(4.0, 4.0, 20.0, 6.0, 24.0, 25.0, 6.0, 22.0, 4.0, 4.0))
    add("three_collinear_points", 32, 32, f(2.0, 2.0, 10.0, 6.0, 18.0, 10.0, 20.0, 28.0, 3.0, 20.0))
    add("half_integer_coordinates", 40, 36, f(2.5, 3.5, 30.5, 4.5, 33.5, 35.5, 10.5, 38.5, 1.5, 20.5))
    add("integer_coordinates", 40, 36, f(2.0, 3.0, 30.0, 4.0, 33.0, 35.0, 10.0, 38.0, 1.0, 20.0))
    add("bow_tie", 40, 40, f(5.0, 5.0, 35.0, 33.0, 35.0, 6.0, 4.0, 34.0))
    add("three_parts_two_overlap", 48, 56, regular(18.0, 20.0, 12.0, 7), regular(28.0, 24.0, 11.0, 9, 0.3), f(40.0, 30.0, 54.0, 31.0, 47.0, 46.0))
    add("circle_1500_vertices", 96, 96, regular(47.3, 49.1, 40.2, 1500))
    add("long_edge_star", 257, 515, star(250.0, 130.0, 60.0, 420.0, 5))
    return C


def random_cases(rng, n):
    out = []
    for i in range(n):
        h, w = int(rng.integers(2, 70)), int(rng.integers(2, 70))
        parts = []
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(3, 12))
            p = rng.uniform(-0.3, 1.3, size=(k, 2)) * np.array([w, h])
            step = float(rng.choice([0.0, 0.5, 1.0]))               # free, half-integer or integer coordinates
            if step:
                p = np.round(p / step) * step
            parts.append(p.reshape(-1))
        out.append(("random_%02d" % i, h, w, parts))
    return out


def urle_cases(rng):
    out = []
    m = (rng.uniform(size=(9 * 17,)) < 0.4).astype(np.uint8)
    m[0] = 1                                                        # starts with ones: the first count is 0
    m[-1] = 0
    out.append(("leading_zero_count", 9, 17, m))
    m = np.zeros((12 * 11,), np.uint8)
    m[5:40], m[50:70], m[90:] = 1, 1, 1                             # 0 1 0 1 0 1: six counts
    out.append(("even_number_of_counts", 12, 11, m))
    m = np.zeros((12 * 11,), np.uint8)
    m[5:40], m[50:70] = 1, 1                                        # 0 1 0 1 0: five counts
    out.append(("odd_number_of_counts", 12, 11, m))
    out.append(("all_zero", 7, 19, np.zeros((7 * 19,), np.uint8)))
    res = []
    for name, h, w, m in out:
        edges = np.flatnonzero(np.diff(m)) + 1
        c = np.diff(np.concatenate([[0], edges, [len(m)]]))
        if m[0]:
            c = np.concatenate([[0], c])
        assert np.array_equal(PG.decode(c, h * w), m)
        res.append((name, h, w, c.astype(np.uint32), m))
    return res


def eval_set(rng):
    """about 6 images, 3 categories; ground truth as polygons (some of several parts) and one crowd region as uncompressed counts;
    detections as compressed RLE: jittered copies of the ground truth and a few false positives, rasterised by the reference"""
    sizes = [(48, 64), (60, 40), (33, 47), (64, 64), (50, 70), (41, 39)]
    images = [{"id": 100 + i, "height": h, "width": w} for i, (h, w) in enumerate(sizes)]
    gt_poly, gt_rle, dt = [], [], []
    for im in images:
        h, w, img = im["height"], im["width"], im["id"]
        for j in range(int(rng.integers(2, 5))):
            cat = int(rng.integers(1, 4))
            cx, cy, r = rng.uniform(0.1, 0.9) * w, rng.uniform(0.1, 0.9) * h, rng.uniform(0.12, 0.3) * min(h, w)
            parts = [np.round(regular(cx, cy, r, int(rng.integers(4, 10)), float(rng.uniform(0, 1))) * 2) / 2]
            if j == 1:                                              # a second part, apart from or overlapping the first
                parts.append(np.round(regular(cx + r, cy + 0.5 * r, 0.6 * r, 5) * 2) / 2)
            _pc, _pa, _mc, _ma, ms = ref_record(parts, h, w)
            rec = {"id": len(gt_poly) + 1, "image_id": img, "category_id": cat, "iscrowd": 0}
            gt_poly.append(dict(rec, segmentation=[[float(v) for v in p] for p in parts]))
            gt_rle.append(dict(rec, segmentation={"size": [h, w], "counts": ms.decode("ascii")}))
            for _ in range(int(rng.integers(1, 3))):
                q = [p + rng.uniform(-0.12, 0.12) * r * 2 for p in parts]
                ds = ref_record(q, h, w)[4]
                dcat = cat if rng.uniform() < 0.8 else int(rng.integers(1, 4))
                dt.append({"image_id": img, "category_id": dcat, "score": round(float(rng.uniform(0.05, 1.0)), 3),
                           "segmentation": {"size": [h, w], "counts": ds.decode("ascii")}})
        fp = ref_record([regular(rng.uniform(0, w), rng.uniform(0, h), 0.2 * min(h, w), 6)], h, w)[4]
        dt.append({"image_id": img, "category_id": int(rng.integers(1, 4)), "score": round(float(rng.uniform(0.05, 0.6)), 3),
                   "segmentation": {"size": [h, w], "counts": fp.decode("ascii")}})
    # one crowd region, as an annotation file stores it: uncompressed counts
    im = images[3]
    h, w = im["height"], im["width"]
    m = np.zeros((w, h), np.uint8)                                  # (column-major element order: [x][y])
    m[10:40, 5:30] = 1
    m[20:50, 25:45] = 1
    m = m.reshape(-1)
    edges = np.flatnonzero(np.diff(m)) + 1
    c = np.diff(np.concatenate([[0], edges, [len(m)]]))
    _a, cs = ref_from_counts(c, h, w)
    rec = {"id": len(gt_poly) + 1, "image_id": im["id"], "category_id": 2, "iscrowd": 1}
    gt_poly.append(dict(rec, segmentation={"size": [h, w], "counts": [int(v) for v in c]}))
    gt_rle.append(dict(rec, segmentation={"size": [h, w], "counts": cs.decode("ascii")}))
    for k in range(2):                                              # two detections inside the crowd region
        q = regular(18.0 + 14 * k, 22.0 + 8 * k, 7.0, 8)
        dt.append({"image_id": im["id"], "category_id": 2, "score": 0.7 - 0.2 * k,
                   "segmentation": {"size": [h, w], "counts": ref_record([q], h, w)[4].decode("ascii")}})
    return images, gt_poly, gt_rle, dt, [1, 2, 3]


def main():
    global L
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "polymask.npz"))
    a = ap.parse_args()
    assert maskapi_ref.available(), "run `make -C oracle` first"
    L = _bind()
    rng = np.random.default_rng(20240917)
    cases = named_cases() + random_cases(rng, 24)
    names, xy, voff, poff, size = [], [], [0], [0], []
    pc, pco, pa, rc, rco, ra = [], [0], [], [], [0], []
    by_name = {}
    for name, h, w, parts in cases:
        p_counts, p_area, m_counts, m_area, _s = ref_record(parts, h, w)
        names.append(name)
        size.append((h, w))
        for p, c, ar in zip(parts, p_counts, p_area):
            xy.append(p)
            voff.append(voff[-1] + len(p) // 2)
            pc.append(c)
            pco.append(pco[-1] + len(c))
            pa.append(ar)
            assert int(c.sum()) == h * w
        poff.append(poff[-1] + len(parts))
        rc.append(m_counts)
        rco.append(rco[-1] + len(m_counts))
        ra.append(m_area)
        by_name[name] = (h, w, parts, [PG.decode(c, h * w) for c in p_counts], PG.decode(m_counts, h * w))
    urle = urle_cases(rng)
    images, gt_poly, gt_rle, dt, cats = eval_set(rng)
    js = lambda v: np.frombuffer(json.dumps(v).encode(), np.uint8)
    ustr, uarea = [], []
    for _name, h, w, c, m in urle:
        ar, s = ref_from_counts(c, h, w)
        assert ar == int(m.sum())
        ustr.append(s.decode("ascii"))
        uarea.append(ar)
    out = {"names": js(names), "xy": np.concatenate(xy), "part_vertex_off": np.array(voff, np.int64), "rec_part_off": np.array(poff, np.int64),
           "size": np.array(size, np.int64), "part_counts": np.concatenate(pc), "part_counts_off": np.array(pco, np.int64),
           "part_area": np.array(pa, np.int64), "rec_counts": np.concatenate(rc), "rec_counts_off": np.array(rco, np.int64),
           "rec_area": np.array(ra, np.int64), "urle_names": js([u[0] for u in urle]), "urle_size": np.array([(u[1], u[2]) for u in urle], np.int64),
           "urle_counts": np.concatenate([u[3] for u in urle]), "urle_off": np.cumsum([0] + [len(u[3]) for u in urle]).astype(np.int64),
           "urle_area": np.array(uarea, np.int64), "urle_strings": js(ustr), "eval_images": js(images), "eval_gt_poly": js(gt_poly),
           "eval_gt_rle": js(gt_rle), "eval_dt": js(dt), "eval_cats": js(cats)}

    # ---- the cases the tests rely on ----
    for name in ("size_13x11", "size_300x7"):
        h, w = by_name[name][:2]
        assert (h * w) % 64 and h * w > 128 and by_name[name][4].any()
    assert by_name["one_word_column"][:2] == (64, 3) and by_name["h_is_1"][0] == 1 and by_name["w_is_1"][1] == 1
    assert by_name["h_is_1"][4].any() and by_name["w_is_1"][4].any()
    h, w, parts = by_name["outside_every_side"][:3]
    p = parts[0].reshape(-1, 2)
    assert (p[:, 0] < 0).any() and (p[:, 0] > w).any() and (p[:, 1] < 0).any() and (p[:, 1] > h).any()
    h, w, parts = by_name["clamped_to_h_mid_column"][:3]
    x, y = PG.toggles(parts[0], h, w)
    assert ((y == h) & (x > 0) & (x < w - 1)).any(), "a crossing clamped to y == h in a middle column"
    h, w, parts = by_name["position_hw_dropped"][:3]
    x, y = PG.toggles(parts[0], h, w)
    assert ((y == h) & (x == w - 1)).any(), "a position equal to h * w"
    assert not by_name["entirely_outside"][4].any() and ra[names.index("entirely_outside")] == 0
    p = by_name["repeated_consecutive_vertex"][2][0].reshape(-1, 2)
    assert any((p[j] == p[j + 1]).all() for j in range(len(p) - 1))
    p = by_name["repeated_first_last_vertex"][2][0].reshape(-1, 2)
    assert (p[0] == p[-1]).all()
    p = by_name["three_collinear_points"][2][0].reshape(-1, 2)
    assert (p[1] - p[0])[0] * (p[2] - p[1])[1] == (p[1] - p[0])[1] * (p[2] - p[1])[0]
    assert (by_name["half_integer_coordinates"][2][0] % 1 == 0.5).all() and (by_name["integer_coordinates"][2][0] % 1 == 0).all()
    assert by_name["bow_tie"][4].any()
    _h, _w, parts, pm, mm = by_name["three_parts_two_overlap"]
    assert len(parts) == 3 and np.array_equal(mm, pm[0] | pm[1] | pm[2]) and not np.array_equal(mm, pm[0] ^ pm[1] ^ pm[2])
    assert len(by_name["circle_1500_vertices"][2][0]) == 3000 and by_name["circle_1500_vertices"][:2] == (96, 96)
    h, w, parts = by_name["long_edge_star"][:3]
    assert (h, w) == (257, 515) and len(PG.walk(parts[0])[0]) > 3000
    un = [u[0] for u in urle]
    assert urle[un.index("leading_zero_count")][3][0] == 0
    assert len(urle[un.index("odd_number_of_counts")][3]) % 2 == 1 and len(urle[un.index("even_number_of_counts")][3]) % 2 == 0
    assert list(urle[un.index("all_zero")][3]) == [7 * 19]
    assert len(images) == 6 and sorted(set(r["category_id"] for r in gt_poly)) == [1, 2, 3]
    assert sum(1 for r in gt_poly if isinstance(r["segmentation"], dict)) == 1 and any(len(r["segmentation"]) > 1 for r in gt_poly
                                                                                      if isinstance(r["segmentation"], list))
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes): %d polygon records, %d parts" % (a.out, os.path.getsize(a.out), len(names), len(pa)))


if __name__ == "__main__":
    main()
