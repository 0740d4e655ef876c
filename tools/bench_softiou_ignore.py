#!/usr/bin/env python
"""Per-launch times of the soft-IoU sums and backward WITH an ignore map (rsis_softiou_sums_ignore / rsis_softiou_bwd_ignore) against the
plain entry points on the same tensors, in the same run, alternating:
  B=32, T=10, G=20, 256 x 256   (the bench batch: ones-row kernel)          B=8, T=20, G=20, 512 x 1024   (the Cityscapes map)
and, with --tiled, B=8, T=64, G=64, 256 x 256 and B=4, T=128, G=128, 256 x 256 (the tiled kernel, NG = 2 and 4).
ms and GB/s against the bytes the pass must move from memory: sums 4 (T + G) N B (+ N B for the map), backward 4 * 3 T N B (+ N B: the T
prediction rows of an image re-read the map's bytes from L2).  Map: one rectangle covering 15 % of each image.
Device times: HIP events around `reps` launches, min..max of five windows.   python tools/bench_softiou_ignore.py [--tiled]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from rsis_amd import _lib as A


def ev_time(fns, reps, windows=5):
    """min..max ms per launch of each fn, the windows of the fns alternating"""
    for f in fns:
        f(); f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(windows):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            torch.cuda.synchronize()
            t[k].append(a.elapsed_time(b) / reps)
    return [(min(v), max(v)) for v in t]


def main():
    shapes = [(32, 10, 20, 256, 256), (8, 20, 20, 512, 1024)]
    if "--tiled" in sys.argv:
        shapes += [(8, 64, 64, 256, 256), (4, 128, 128, 256, 256)]
    L, p, st = A.lib(), A.ptr, A.stream
    g = torch.Generator("cuda").manual_seed(0)
    for B, T, G, H, W in shapes:
        N = H * W
        logits = torch.randn(B, T, N, device="cuda", generator=g) * 2
        y = (torch.rand(B, G, N, device="cuda", generator=g) < 0.3).float()
        ign = torch.zeros(B, H, W, dtype=torch.uint8, device="cuda")
        for b in range(B):
            y0, x0 = (37 * b) % (H // 2), (53 * b) % (W // 2)
            ign[b, y0:y0 + int(0.4 * H), x0:x0 + int(0.375 * W)] = 1
        ign = ign.view(B, N)
        perm = torch.stack([torch.randperm(max(T, G), device="cuda", generator=g) % G for _ in range(B)]).contiguous()
        ca, cb = torch.randn(B, T, device="cuda", generator=g) / N, torch.randn(B, T, device="cuda", generator=g) / N
        S, d = torch.empty(B, T + 1, G + 1, device="cuda"), torch.empty_like(logits)
        sums = lambda m: (lambda: A.check(L.rsis_softiou_sums_ignore(p(logits), p(y), p(m), p(S), B, T, G, N, st()), "sums"))    # noqa: E731
        bwd = lambda m: (lambda: A.check(L.rsis_softiou_bwd_ignore(p(logits), p(y), p(m), p(perm), perm.shape[1], p(ca), p(cb), p(d),    # noqa: E731
                                                                   B, T, G, N, st()), "bwd"))
        reps = 20
        (s0, s1), (b0, b1) = ev_time([sums(None), sums(ign)], reps), ev_time([bwd(None), bwd(ign)], reps)
        sb, bb = 4.0 * (T + G) * N * B, 12.0 * T * N * B
        print("B=%d T=%d G=%d %dx%d  (ignored: %.1f %% of the pixels)" % (B, T, G, H, W, 100.0 * float(ign.float().mean())))
        print("  sums  plain %.4f..%.4f ms %7.1f GB/s | ignore %.4f..%.4f ms %7.1f GB/s | ignore / plain (min) %.3f   bytes +1/%d"
              % (s0[0], s0[1], sb / s0[0] / 1e6, s1[0], s1[1], (sb + N * B) / s1[0] / 1e6, s1[0] / s0[0], 4 * (T + G)))
        print("  bwd   plain %.4f..%.4f ms %7.1f GB/s | ignore %.4f..%.4f ms %7.1f GB/s | ignore / plain (min) %.3f   bytes +1/%d"
              % (b0[0], b0[1], bb / b0[0] / 1e6, b1[0], b1[1], (bb + N * B) / b1[0] / 1e6, b1[0] / b0[0], 12 * T), flush=True)
        del logits, y, d


if __name__ == "__main__":
    main()
