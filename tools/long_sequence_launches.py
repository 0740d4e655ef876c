#!/usr/bin/env python
"""Per-launch times of the soft-IoU sums and the assignment at long sequences against the paths they replace (B = 32, N = 65536):
  rsis_softiou_sums at (T, G) = (10, 20) ... (128, 128): us, GB/s against the bytes 4 (T + G) N B, TFLOP/s (2 T G N B) against the
    157.3 of the exact-f32 MFMA; next to it utils.hungarian.softIoU_matrix (sigmoid + torch.bmm + the plain sums) on the same tensors
  rsis_assign_min_cost at (G, T) = (64, 20), (72, 36), (128, 128) on uniform costs and on the reference's masked structure (invalid
    pairs = 10, 37 % of the slots valid); next to it the host path on the same scores: D2H + scipy + H2D, wall time with a synchronise around it.
Device times: HIP events around 20 launches, min..max of three windows.   python tools/long_sequence_launches.py"""
import sys
import time
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rsis_amd import ops
from rsis_amd.utils.hungarian import match_indices, softIoU_matrix


def ev_time(fn, reps):
    fn(); fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3 / reps)
    return min(t), max(t)


B, N = 32, 65536
g = torch.Generator("cuda").manual_seed(0)
print("rsis_softiou_sums vs softIoU_matrix (bmm), B=%d N=%d: us min..max of 3 windows" % (B, N))
for T, G in [(10, 20), (10, 40), (40, 40), (64, 64), (128, 128)]:
    logits = torch.randn(B, T, N, device="cuda", generator=g) * 2
    y = (torch.rand(B, G, N, device="cuda", generator=g) < 0.3).float()
    reps = 20
    k = ev_time(lambda: ops.softiou_sums(logits, y), reps)
    m = ev_time(lambda: softIoU_matrix(y, logits), reps)
    byts = 4.0 * (T + G) * N * B
    fl = 2.0 * T * G * N * B
    print("T=%3d G=%3d  sums %8.1f..%8.1f us  %7.1f GB/s  %6.2f TFLOP/s (%.1f%% of 157.3) | bmm path %8.1f..%8.1f us"
          % (T, G, k[0], k[1], byts / k[0] / 1e3, fl / k[0] / 1e6, 100 * fl / k[0] / 1e6 / 157.3, m[0], m[1]), flush=True)
    del logits, y

print("rsis_assign_min_cost vs D2H + scipy + H2D, B=%d" % B)
for G, T in [(64, 20), (72, 36), (128, 128)]:
    for kind in ("uniform", "masked"):
        sc = np.random.default_rng(G + T).uniform(0, 1, (B, G, T)).astype(np.float32)
        if kind == "masked":
            n_inst = int(0.37 * G)
            sw = np.zeros(G, np.float32)
            sw[:n_inst] = 1
            valid = sw[None, :, None] * sw[None, None, :T]
            sc = sc * valid + (1 - valid) * 10
        s = torch.from_numpy(sc).cuda()
        k = ev_time(lambda: ops.assign_min_cost(s), 20)

        def host():
            return torch.from_numpy(match_indices(s)).to(s.device)
        host(); torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        print("G=%3d T=%3d %-8s device %8.1f..%8.1f us | host round trip %8.1f..%8.1f us" % (G, T, kind, k[0], k[1], min(ts), max(ts)), flush=True)
