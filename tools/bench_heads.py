"""Times the class / stop heads kernels alone (csrc/losses.hip): the small family (rsis_heads_fwd / rsis_heads_bwd) where it accepts the
call, and the wide family (rsis_heads_wide_fwd / rsis_heads_wide_bwd: two launches), forward and backward, at

    rows 320 and 640 at 21 classes, rows 640 at 81 classes, rows 640 at 256 classes      (K = 248: the decoder's heads at hidden 128)

    python tools/bench_heads.py [--inner 200] [--runs 9]

HIP events around `--inner` back-to-back launches of one kernel (a single launch of ~10 us is below what an event pair resolves), the two
families alternating run by run, after a warm-up of every shape; the median over `--runs` of the time per call, and the spread (min,
max).  The parameter gradients are accumulated into (+=), so their buffers drift over the launches: the time does not depend on the
values.  One JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CS = [128, 64, 32, 16, 8]
SHAPES = [(320, 21), (640, 21), (640, 81), (640, 256)]


def time_us(fn, inner, runs_out):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    runs_out.append(1e3 * a.elapsed_time(b) / inner)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--runs", type=int, default=9)
    o = ap.parse_args(argv)
    from rsis_amd import _lib as A
    from rsis_amd import ops
    L = A.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *sh: torch.randn(*sh, device="cuda", generator=g)
    K = sum(CS)
    for rows, ncls in SHAPES:
        sides, dsides = [rnd(rows, c) for c in CS], [torch.empty(rows, c, device="cuda") for c in CS]
        Wc, bc, Ws, bs = rnd(ncls, K) / K ** 0.5, rnd(ncls), rnd(1, K) / K ** 0.5, rnd(1)
        probs, stop = torch.empty(rows, ncls, device="cuda"), torch.empty(rows, 1, device="cuda")
        dprobs, dstop = rnd(rows, ncls), rnd(rows, 1)
        hb = [torch.zeros_like(t) for t in (Wc, bc, Ws, bs)]
        scratch = torch.empty(rows * (ncls + 1), device="cuda")
        sp, ia, st = A.ptr_array(sides), A.int_array(CS), A.stream()
        w = (A.ptr(Wc), A.ptr(bc), ncls, A.ptr(Ws), A.ptr(bs), A.ptr(probs), A.ptr(stop), st)
        bw = (sp, ia, 5, rows, A.ptr(Wc), ncls, A.ptr(Ws), A.ptr(probs), A.ptr(dprobs), A.ptr(dstop), A.ptr_array(dsides), A.ptr(hb[0]), A.ptr(hb[1]),
              A.ptr(hb[2]), A.ptr(hb[3]))
        calls = {"wide_fwd": lambda: A.check(L.rsis_heads_wide_fwd(None, None, None, sp, ia, 5, rows, *w), "rsis_heads_wide_fwd"),
                 "wide_bwd": lambda: A.check(L.rsis_heads_wide_bwd(*bw, A.ptr(scratch), scratch.numel(), st), "rsis_heads_wide_bwd")}
        if ops.heads_family(rows, K, ncls) == "small":
            calls["small_fwd"] = lambda: A.check(L.rsis_heads_fwd(sp, ia, 5, rows, *w), "rsis_heads_fwd")
        if ops.heads_family(rows, K, ncls, backward=True) == "small":
            calls["small_bwd"] = lambda: A.check(L.rsis_heads_bwd(*bw, st), "rsis_heads_bwd")
        for fn in calls.values():                 # warm-up: code objects, the forward fills probs for the backward
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(o.runs):                   # the families alternate inside a run
            for k in sorted(calls):
                time_us(calls[k], o.inner, ts[k])
        res = {"rows": rows, "K": K, "ncls": ncls, "dispatch": {"fwd": ops.heads_family(rows, K, ncls), "bwd": ops.heads_family(rows, K, ncls, backward=True)}}
        for k in sorted(ts):
            res[k + "_us"] = {"median": round(float(np.median(ts[k])), 2), "min": round(min(ts[k]), 2), "max": round(max(ts[k]), 2)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
