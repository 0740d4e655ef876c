"""Writes tests/golden/cvppp.npz: a dozen small pairs of label images with the counts and the six CVPPP scores that the float64 numpy
statement of the definitions (tests/cvppp_golden.py) gives for them.  Deterministic; no GPU.

    python tools/make_golden_cvppp.py [--out tests/golden/cvppp.npz]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cvppp_golden as G  # noqa: E402


def blobs(rng, h, w, k, first=1, radius=(3.0, 7.0)):
    """k elliptical leaves labelled first .. first + k - 1 on background 0; later leaves paint over earlier ones"""
    yy, xx = np.mgrid[0:h, 0:w]
    lab = np.zeros((h, w), np.uint8)
    for n in range(k):
        cy, cx = rng.uniform(0.1, 0.9) * h, rng.uniform(0.1, 0.9) * w
        a, b, th = rng.uniform(*radius), rng.uniform(*radius), rng.uniform(0, np.pi)
        u = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th)
        v = -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
        lab[(u / a) ** 2 + (v / b) ** 2 <= 1.0] = first + n
    return lab


def shifted(a, dy, dx):
    out = np.zeros_like(a)
    h, w = a.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = a[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def cases():
    from PIL import Image
    from rsis_amd.dataloader.leaves import synthesize_leaves_dir
    rng = np.random.default_rng(20261016)
    out = []
    a = blobs(rng, 64, 80, 6)
    out.append(("identical", a, a.copy()))
    out.append(("gap_0_1_3_vs_0_1_2", np.array([[0, 0, 1, 3]], np.uint8), np.array([[0, 0, 1, 2]], np.uint8)))
    g = blobs(rng, 48, 56, 5)
    r = g.copy()
    r[r == 2] = 0
    r[r == 4] = 7                                                  # values {0, 1, 3, 5, 7}: gaps inside the range
    out.append(("gaps_larger", r, g))
    out.append(("all_zero_result_tiny", np.zeros((2, 2), np.uint8), np.array([[0, 1], [1, 2]], np.uint8)))
    out.append(("all_zero_result", np.zeros((40, 52), np.uint8), blobs(rng, 40, 52, 4)))
    out.append(("both_constant", np.full((2, 3), 5, np.uint8), np.full((2, 3), 9, np.uint8)))
    g = blobs(rng, 50, 50, 5)
    out.append(("background_7", (shifted(g, 1, -2).astype(np.int64) + 7).astype(np.uint8), (g.astype(np.int64) + 7).astype(np.uint8)))
    g = (blobs(rng, 33, 47, 1) * 255).astype(np.uint8)
    out.append(("labels_0_and_255", shifted(g, 2, 1), g))
    g = blobs(rng, 96, 112, 40, radius=(3.0, 6.0))
    r = shifted(g, 1, 1)
    r[r == 17] = 16                                                # two leaves merged, one missed
    r[r == 30] = 0
    out.append(("forty_leaves", r, g))
    with tempfile.TemporaryDirectory() as d:
        synthesize_leaves_dir(d, n=1, size=(96, 112), seed=3)
        g = np.array(Image.open(os.path.join(d, "plant000_label.png")))
    out.append(("synthesized_shifted", shifted(g, -3, 2), g))
    out.append(("other_size_nearest", blobs(rng, 31, 45, 4), blobs(rng, 60, 72, 4)))
    out.append(("whole_range", rng.integers(0, 256, (37, 41)).astype(np.uint8), rng.integers(0, 256, (37, 41)).astype(np.uint8)))
    out.append(("over_segmented", blobs(rng, 64, 64, 12), blobs(rng, 64, 64, 3, radius=(8.0, 14.0))))
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cvppp.npz"))
    a = p.parse_args(argv)
    z, names = {}, []
    for k, (name, r, g) in enumerate(cases()):
        assert r.dtype == np.uint8 and g.dtype == np.uint8 and max(r.shape[0], g.shape[0]) <= 96 and max(r.shape[1], g.shape[1]) <= 112
        rr = G.nearest_resize(r, *g.shape) if r.shape != g.shape else r
        t = G.counts(rr, g).reshape(-1)
        cell = np.nonzero(t)[0]
        names.append(name)
        z["c%d_in" % k], z["c%d_gt" % k] = r, g
        z["c%d_cell" % k], z["c%d_count" % k] = cell.astype(np.int32), t[cell].astype(np.int64)
        z["c%d_scores" % k] = G.scores_from_counts(t.reshape(256, 256))
        print("%-22s %s" % (name, " ".join("%.6f" % v for v in z["c%d_scores" % k])))
    z["names"] = np.frombuffer("\n".join(names).encode(), np.uint8)
    np.savez_compressed(a.out, **z)
    print("%s: %d cases, %d bytes" % (a.out, len(names), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
