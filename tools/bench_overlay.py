"""Times the --display compositing (NOTES.md entry on rsis_overlay_masks / rsis_overlay_moments, csrc/overlay.hip):

    python tools/bench_overlay.py [--height 1024] [--width 2048] [--k 20] [--sets 6] [--runs 60]

  masks    : rsis_overlay_masks alone, per launch, and the bytes it must move (image in, image out, k masks) over that time;
  moments  : rsis_overlay_moments alone, per launch, and its k masks of bytes over that time;
  overlay  : display.overlay as eval.py calls it (order / colour upload, both launches);
  host     : what the launches replace: the k byte masks copied to the host, transposed to row-major and blended in numpy (float32), plus
             scipy-free centres of mass -- and the copy alone.
The masks are k ellipses per image of 0.5-6 % of the image each (a Cityscapes frame's instances), column-major bytes as
rsis_mask_resize_threshold writes them.  `--sets` independent (image, masks) sets are cycled so that the working set (sets x (k + 6) x h x w
bytes: 330 MB at the defaults) does not fit the 256 MB Infinity Cache: the rate is then an HBM rate.  Device events around `--runs`
back-to-back launches after `--warmup` of them; one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ellipse_masks(r, k, h, w):
    """(k, w * h) column-major uint8"""
    xx, yy = np.mgrid[0:w, 0:h]
    out = np.zeros((k, w, h), np.uint8)
    for j in range(k):
        area = r.uniform(0.005, 0.06) * h * w
        ar = r.uniform(0.5, 2.0)
        a, b = np.sqrt(area * ar / np.pi), np.sqrt(area / ar / np.pi)
        cy, cx = r.uniform(0.1, 0.9) * h, r.uniform(0.1, 0.9) * w
        out[j] = ((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2 <= 1.0
    return out.reshape(k, w * h)


def events_ms(fn, warmup, runs):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(runs):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / runs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--runs", type=int, default=60)
    ap.add_argument("--host_runs", type=int, default=3)
    a = ap.parse_args(argv)
    from rsis_amd import display
    from rsis_amd._lib import check, lib, ptr, stream
    h, w, k = a.height, a.width, a.k
    r = np.random.default_rng(0)
    host_masks = ellipse_masks(r, k, h, w)
    host_image = r.integers(0, 256, (h, w, 3), dtype=np.uint8)
    images = [torch.as_tensor(np.roll(host_image, 7 * i, axis=1)).cuda() for i in range(a.sets)]
    masks = [torch.as_tensor(np.roll(host_masks, 3 * i, axis=0)).cuda() for i in range(a.sets)]
    outs = [torch.empty_like(images[0]) for _ in range(a.sets)]
    order = torch.arange(k, dtype=torch.int32, device="cuda")
    colors = torch.as_tensor(display.sequence_colors(k)).cuda()
    moments = torch.zeros((k, 3), dtype=torch.int64, device="cuda")
    L = lib()

    def f_masks(i):
        s = i % a.sets
        check(L.rsis_overlay_masks(ptr(images[s]), ptr(masks[s]), k, ptr(order), ptr(colors), k, 0.5, ptr(outs[s]), h, w, stream()), "masks")

    def f_moments(i):
        check(L.rsis_overlay_moments(ptr(masks[i % a.sets]), k, ptr(order), k, h, w, ptr(moments), stream()), "moments")

    def f_overlay(i):
        display.overlay(images[i % a.sets], masks[i % a.sets], order, colors)

    t_masks = events_ms(f_masks, a.warmup, a.runs)
    t_moments = events_ms(f_moments, a.warmup, a.runs)
    t_overlay = events_ms(f_overlay, a.warmup, a.runs)
    bytes_masks = (k + 6) * h * w
    bytes_moments = k * h * w

    # the host alternative on the same data (set 0), and that its result is the device's
    def host(i):
        m = masks[0].cpu().numpy().reshape(k, w, h)
        v = host_image.astype(np.float32)
        cols = display.sequence_colors(k).astype(np.float32)
        centres = []
        for j in range(k):
            on = m[j].T != 0
            v[on] += np.float32(0.5) * (cols[j] - v[on])
            ys, xs = np.nonzero(on)
            centres.append((ys.mean(), xs.mean()) if ys.size else None)
        return np.floor(v + np.float32(0.5)).astype(np.uint8), centres

    t_host, t_copy = [], []
    for i in range(a.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        masks[0].cpu()
        t1 = time.perf_counter()
        ref, centres = host(i)
        t2 = time.perf_counter()
        t_copy.append((t1 - t0) * 1e3)
        t_host.append((t2 - t1) * 1e3)
    f_masks(0)
    f_moments(0)
    same = bool((outs[0].cpu().numpy() == ref).all())
    mom = moments.cpu().numpy()
    same_c = all(c is None or (abs(m[1] / m[0] - c[0]) < 1e-6 and abs(m[2] / m[0] - c[1]) < 1e-6) for m, c in zip(mom, centres))
    out = {"overlay": {"h": h, "w": w, "k": k, "sets": a.sets, "coverage_mean": round(float((host_masks != 0).mean()), 4),
                       "masks_ms": round(t_masks, 4), "masks_bytes": bytes_masks, "masks_TBps": round(bytes_masks / t_masks / 1e9, 3),
                       "moments_ms": round(t_moments, 4), "moments_bytes": bytes_moments,
                       "moments_TBps": round(bytes_moments / t_moments / 1e9, 3), "overlay_call_ms": round(t_overlay, 4),
                       "host_copy_ms": round(min(t_copy), 2), "host_blend_ms": round(min(t_host), 2),
                       "host_total_ms": round(min(t_copy) + min(t_host), 2),
                       "speedup_vs_host": round((min(t_copy) + min(t_host)) / t_overlay, 1), "same_pixels": same, "same_centres": bool(same_c)}}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
