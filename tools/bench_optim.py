#!/usr/bin/env python
"""Time the three fused flat optimizer steps (rsis_adam_step, rsis_sgd_step, rsis_rmsprop_step) over ONE flat range of the model's
parameter count (48.6 M) on the GPU, next to a copy of the same range as the bandwidth yardstick.
    python tools/bench_optim.py [--n 48600000] [--iters 20] [--offset 0]
Prints, per rule, the median launch time (HIP events) and the bytes it must move over that time: Adam reads p, g, m, v and writes
p, m, v (28 B per parameter); SGD and RMSprop read p, g and their one state buffer and write p and the buffer (20 B); the copy reads
and writes 4 B each.  --offset starts the range that many floats into the buffers (the unaligned-head path)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _median_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=48600000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--offset", type=int, default=0)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: no GPU visible (a CPU run cannot time a kernel)")
    from rsis_amd import ops
    n, off = o.n, o.offset
    gen = torch.Generator(device="cuda").manual_seed(0)
    bufs = [torch.randn(n + off, device="cuda", generator=gen) * 1e-2 for _ in range(4)]
    p, g, m, v = [b[off:off + n] for b in bufs]
    v.abs_()
    dst = torch.empty_like(p)
    rules = [
        ("adam", 28, lambda: ops.adam_step_flat(p, g, m, v, 1e-4, 0.9, 0.999, 1e-8, 1e-6, 10, 1.0, bump=False)),
        ("sgd", 20, lambda: ops.sgd_step_flat(p, g, m, 1e-4, 0.9, 1e-6, 1.0, bump=False)),
        ("rmsprop", 20, lambda: ops.rmsprop_step_flat(p, g, v, 1e-4, 0.99, 1e-8, 1e-6, 1.0, bump=False)),
        ("copy", 8, lambda: dst.copy_(p)),
    ]
    out = {"n": n, "offset": off, "device": torch.cuda.get_device_name(0)}
    for name, bpp, fn in rules:
        ms, ms_min = _median_ms(fn, o.iters)
        out[name] = {"ms": round(ms, 4), "ms_min": round(ms_min, 4), "bytes_per_param": bpp, "TB_s": round(bpp * n / (ms * 1e-3) / 1e12, 3)}
        print("%-8s %7.4f ms (min %.4f)  %5.1f MB moved  %.2f TB/s" % (name, ms, ms_min, bpp * n / 1e6, out[name]["TB_s"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
