"""Times of the CVPPP label-image scoring launches (rsis_amd/csrc/labeleval.hip; NOTES.md (71)).

    python tools/bench_labeleval.py                # on the GPU: the three workloads below, one JSON line each
    python tools/bench_labeleval.py --resources    # no GPU: the compiler's resource lines of the two kernels (hipcc, gfx950)

Workloads: (a) 128 pairs of 530 x 500 (CVPPP A1 size) with leaf-like labels, (a0) the same with every image 100 % background (every
update of a pair lands on ONE cell), (b) 27 pairs of 2448 x 2048 (A3 size).  Per workload, median of 20 device-event timings after
warm-up: the contingency launch, the scores launch (each with the memset that zeroes its output); host clock around a synchronise for
pool copy + both launches + scores copy; bytes read (2 per pixel: every image byte once) / contingency time, next to a torch copy of
the SAME pool timed in the same run (a copy reads and writes every byte, so its figure is bytes read / time as well); and the float64
numpy statement of tests/cvppp_golden.py on the host over the first --host-pairs pairs, as an informational per-pair time."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def leafy(rng, h, w, k, background):
    lab = np.zeros((h, w), np.uint8)
    if background >= 1.0:
        return lab
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.sqrt((1.0 - background) * h * w / (k * np.pi)) * 1.1
    for n in range(1, k + 1):
        cy, cx, th = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w, rng.uniform(0, np.pi)
        u = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th)
        v = -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
        lab[(u / (1.4 * r)) ** 2 + (v / (0.7 * r)) ** 2 <= 1.0] = n
    return lab


def workload(name, n, h, w, background, distinct):
    """n pairs; `distinct` different images are drawn and cycled (drawing 128 of them says nothing more about the kernel)"""
    import torch
    rng = np.random.default_rng(71)
    base = []
    for _ in range(distinct):
        g = leafy(rng, h, w, int(rng.integers(4, 12)), background)
        base.append((np.roll(g, (3, -2), (0, 1)).copy(), g))
    pairs = [base[k % distinct] for k in range(n)]
    return name, [torch.from_numpy(a) for a, _g in pairs], [torch.from_numpy(g) for _a, g in pairs]


def events(fn, reps=20, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def run(name, ins, gts, host_pairs):
    import torch
    import cvppp_golden as G
    from rsis_amd import cvppp_eval as E
    dev = torch.device("cuda")
    pool, jobs, n, blocks = E._pool(ins, gts, 16, dev)
    host_pool, host_jobs = pool.cpu().pin_memory(), jobs.cpu()
    counts = E._launch_contingency(pool, jobs, n, blocks)
    pixels = int(sum(g.numel() for g in gts))
    t_cont = events(lambda: E._launch_contingency(pool, jobs, n, blocks))
    t_scores = events(lambda: E._launch_scores(counts, jobs, n))
    dst = torch.empty_like(pool)
    t_copy = events(lambda: dst.copy_(pool))

    def whole():
        p, j = host_pool.to(dev, non_blocking=True), host_jobs.to(dev, non_blocking=True)
        return E._launch_scores(E._launch_contingency(p, j, n, blocks), j, n).cpu()
    wall = []
    for _ in range(8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = whole()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    k = min(host_pairs, n)
    t0 = time.perf_counter()
    want = G.score_pairs([a.numpy() for a in ins[:k]], [g.numpy() for g in gts[:k]])
    t_host = (time.perf_counter() - t0) * 1e3 / max(k, 1)
    assert G.same_scores(s[:k].numpy(), want), "device scores differ from the numpy statement"
    bg = float(np.mean([float((g == g.min()).float().mean()) for g in gts[:k]]))
    out = {"workload": name, "pairs": n, "pixels": pixels, "blocks": blocks, "background_fraction": round(bg, 3),
           "contingency_ms": round(t_cont, 4), "scores_ms": round(t_scores, 4), "both_plus_copies_wall_ms": round(float(np.median(wall[2:])), 3),
           "bytes_read": 2 * pixels, "contingency_TBps": round(2 * pixels / (t_cont * 1e-3) / 1e12, 3),
           "torch_copy_same_pool_ms": round(t_copy, 4), "torch_copy_TBps_read": round(pool.numel() / (t_copy * 1e-3) / 1e12, 3),
           "numpy_statement_host_ms_per_pair": round(t_host, 2), "host_pairs_checked_equal": k}
    print(json.dumps(out), flush=True)
    return out


def resources():
    src = os.path.join(ROOT, "rsis_amd", "csrc", "labeleval.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    keep = ("Function Name", " VGPRs:", "AGPRs", "ScratchSize", "LDS Size", "Occupancy", "TotalSGPRs")
    for line in p.stdout.splitlines():
        if any(k in line for k in keep):
            print(line.split("remark:")[-1].rstrip().replace(" [-Rpass-analysis=kernel-resource-usage]", ""))
    return p.returncode


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--resources", action="store_true")
    p.add_argument("--host-pairs", type=int, default=4)
    a = p.parse_args(argv)
    if a.resources:
        return resources()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_labeleval.py needs the GPU (or --resources)")
    res = [run(*workload("a_128x530x500_leaves", 128, 530, 500, 0.7, 16), a.host_pairs),
           run(*workload("a0_128x530x500_all_background", 128, 530, 500, 1.0, 1), a.host_pairs),
           run(*workload("b_27x2448x2048_leaves", 27, 2048, 2448, 0.7, 3), a.host_pairs)]
    print(json.dumps({"all_background_over_leaves_contingency": round(res[1]["contingency_ms"] / res[0]["contingency_ms"], 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
