"""Time of the polygon -> bit-row launch (rsis_poly_to_bits, rsis_amd/csrc/polymask.hip) on a synthetic set shaped like the polygons
of a COCO validation file (NOTES.md): 5000 records of 1 - 3 parts, 10 - 60 vertices per part, images of 480 x 640.

    python tools/bench_polymask.py [--records 5000]

Prints one JSON line: the grouped launch alone (device events over repeated launches, tables already on the device), the whole
cocoeval.poly_to_bits call (host tables + copies + launch), and -- where oracle/_ref/libmaskapi_ref.so has been built -- the same set
through that library's rleFrPoly + rleMerge on one CPU core, with the areas of both compared.  Not part of bench.py."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 480, 640


def make_set(n, seed=11):
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        parts = []
        for _p in range(int(rng.integers(1, 4))):
            k = int(rng.integers(10, 61))
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            r = rng.uniform(8, 120) * rng.uniform(0.7, 1.3, size=k)
            a = np.sort(rng.uniform(0, 2 * np.pi, size=k))
            parts.append(np.round(np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1).reshape(-1), 2))
        recs.append(parts)
    return recs


class _RLE(ctypes.Structure):
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def host_library(recs):
    """-> (seconds, areas) through the reference-built mask library, or None where it has not been built"""
    path = os.path.join(ROOT, "oracle", "_ref", "libmaskapi_ref.so")
    if not os.path.exists(path):
        return None
    L = ctypes.CDLL(path)
    P = ctypes.POINTER(_RLE)
    L.rleFrPoly.argtypes = [P, ctypes.c_void_p, ctypes.c_ulong, ctypes.c_ulong, ctypes.c_ulong]
    L.rleMerge.argtypes = [P, P, ctypes.c_ulong, ctypes.c_int]
    L.rleArea.argtypes = [P, ctypes.c_ulong, ctypes.c_void_p]
    L.rleFree.argtypes = [P]
    for f in (L.rleFrPoly, L.rleMerge, L.rleArea, L.rleFree):
        f.restype = None
    areas = np.zeros((len(recs),), np.uint32)
    t0 = time.perf_counter()
    for j, parts in enumerate(recs):
        R = (_RLE * len(parts))()
        for i, p in enumerate(parts):
            L.rleFrPoly(ctypes.byref(R[i]), p.ctypes.data_as(ctypes.c_void_p), len(p) // 2, H, W)
        M = _RLE()
        L.rleMerge(R, ctypes.byref(M), len(parts), 0)
        L.rleArea(ctypes.byref(M), 1, areas[j:].ctypes.data_as(ctypes.c_void_p))
        for i in range(len(parts)):
            L.rleFree(ctypes.byref(R[i]))
        L.rleFree(ctypes.byref(M))
    return time.perf_counter() - t0, areas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=500)
    a = ap.parse_args()
    import torch
    from rsis_amd import cocoeval as CE
    recs = make_set(a.records)
    sizes = [(H, W)] * len(recs)
    out = {"records": len(recs), "parts": sum(len(r) for r in recs), "vertices": sum(len(p) // 2 for r in recs for p in r), "h": H, "w": W}
    for _ in range(2):                                              # the first call loads the code object
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, area = CE.poly_to_bits(recs, sizes)
        torch.cuda.synchronize()
        out["poly_to_bits_call_s"] = time.perf_counter() - t0
    # the launch alone, on tables built the way poly_to_bits builds them
    words = CE.words_of(H * W)
    ptab, rtab, nv, npart = [], [], 0, 0
    for j, parts in enumerate(recs):
        for p in parts:
            ptab.append((nv, len(p) // 2))
            nv += len(p) // 2
        rtab.append((npart, len(parts), H, W, j * words, words, 0, 0))
        npart += len(parts)
    xd = torch.from_numpy(np.concatenate([p for r in recs for p in r])).cuda()
    pd, rd = torch.from_numpy(np.array(ptab, np.int64)).cuda(), torch.from_numpy(np.array(rtab, np.int64)).cuda()
    n = len(recs)
    scratch = torch.empty((n * words,), dtype=torch.int64, device="cuda")
    bits = torch.empty((n * words,), dtype=torch.int64, device="cuda")
    ar = torch.empty((n,), dtype=torch.int32, device="cuda")
    L = CE.lib()
    launch = lambda: CE.check(L.rsis_poly_to_bits(CE.ptr(xd), nv, CE.ptr(pd), npart, CE.ptr(rd), n, CE.ptr(scratch), CE.ptr(bits), n * words,
                                                  CE.ptr(ar), CE.stream()), "rsis_poly_to_bits")
    for _ in range(3):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    assert torch.equal(ar, area) and torch.equal(bits, torch.cat(rows))
    out["launch_ms"] = ms
    out["launch_us_per_record"] = 1e3 * ms / n
    # row bytes the kernel loads and stores: per record it zeroes scratch and output and reads the output for the area (3 rows), per
    # part it reads the scratch, reads and writes the output and re-zeroes the scratch (4 rows); vertices and toggles are small beside it
    out["row_bytes"] = 8 * words * (3 * n + 4 * npart)
    out["row_GB_per_s"] = out["row_bytes"] / ms / 1e6
    host = host_library(recs)
    if host is not None:
        out["host_library_s"] = host[0]
        out["host_library_us_per_record"] = 1e6 * host[0] / n
        out["areas_equal"] = bool(np.array_equal(host[1].astype(np.int64), area.cpu().numpy().astype(np.int64)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
