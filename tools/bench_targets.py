"""Times the two kernels of the Pascal VOC data path against what they replace (NOTES.md entry on rsis_targets_from_maps):

    python tools/bench_targets.py [--batch 28] [--size 256] [--T 20] [--instances 6] [--runs 20]

  targets : dataloader.targets_from_maps with the per-image loop (use_kernel=False: the code of the parent commit) against the
            grouped kernel (rsis_targets_from_maps), at Pascal's training batch;
  palette : rsis_palette_to_ids against the numpy colour lookup on one 375 x 500 image (the reference's per-pixel dict lookup is
            slower than either).
HIP events around each call (they span the host syncs inside it), `--warmup` calls first, the median of `--runs`.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=28)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--instances", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args(argv)
    from rsis_amd.dataloader.pascal import palette_table
    from rsis_amd.dataloader.targets import targets_from_maps
    from rsis_amd.pascal_precompute import ids_from_colors_numpy, palette_to_ids
    r = np.random.default_rng(0)
    S, B = a.size, a.batch
    # `instances` blobs per image on background 0 (blocks of a coarse grid, so that the areas differ), classes 1..20
    coarse = r.integers(0, a.instances + 1, (B, 16, 16))
    ins = torch.from_numpy(np.kron(coarse, np.ones((S // 16, S // 16), np.int64))).cuda()
    seg = torch.where(ins > 0, (ins * 3) % 20 + 1, torch.zeros_like(ins))
    loop = median_ms(lambda: targets_from_maps(ins, seg, a.T, use_kernel=False), a.warmup, a.runs)
    kern = median_ms(lambda: targets_from_maps(ins, seg, a.T, use_kernel=True), a.warmup, a.runs)
    same = all(torch.equal(p, q) for p, q in zip(targets_from_maps(ins, seg, a.T, use_kernel=False), targets_from_maps(ins, seg, a.T)))
    table = palette_table()
    rgb = table[r.integers(0, len(table), (375, 500)), :3].copy()
    rgb_d, table_d = torch.from_numpy(rgb).cuda(), torch.from_numpy(table).cuda()
    pal_kernel = median_ms(lambda: palette_to_ids(rgb_d, table_d), a.warmup, a.runs)
    t0 = time.perf_counter()
    pal_e2e = palette_to_ids(torch.from_numpy(rgb).cuda(), table_d).cpu().numpy()           # upload + kernel + download
    pal_e2e_ms = 1e3 * (time.perf_counter() - t0)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        want = ids_from_colors_numpy(rgb, table)
        ts.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"targets": {"B": B, "size": S, "T": a.T, "instances": a.instances, "loop_ms": round(loop, 4),
                                  "kernel_ms": round(kern, 4), "speedup": round(loop / kern, 2), "bit_equal": bool(same)},
                      "palette_375x500": {"numpy_ms": round(float(np.median(ts)), 4), "kernel_ms": round(pal_kernel, 4),
                                          "kernel_with_copies_ms": round(pal_e2e_ms, 4), "equal": bool(np.array_equal(pal_e2e, want))}}))


if __name__ == "__main__":
    main()
