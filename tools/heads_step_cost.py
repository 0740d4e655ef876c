#!/usr/bin/env python
"""Training-step time at the COCO shape (`--synthetic -num_classes 81 -batch_size 32 -maxseqlen 20 -gt_maxseqlen 20 -imsize 256`): eager and
captured (GraphedStep), fp32 and bf16, each row in its own process as tools/fallback_cost.py does -- warm-up, then `--steps` timed steps
between device synchronisations.

    python tools/heads_step_cost.py [--steps 12] [--classes 81] [--tree DIR] [--repeat 1]

--tree DIR measures ANOTHER built checkout of this repository with the same script (the parent commit, where 81 classes run the
per-step decoder): the child imports bench / rsis_amd from DIR.  --repeat 2 runs every row twice: the run-to-run spread.  Every row says
whether train.py announced the per-step decoder."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(o):
    sys.path.insert(0, o.tree)
    import time
    import torch
    import bench
    from rsis_amd.modules import FeatureExtractor, RSIS
    from rsis_amd.synthetic import synthetic_batch
    from rsis_amd.train import GraphedStep, build_optimizers, runIter, steps_to_run
    from rsis_amd.utils.objectives import MaskedBCELoss, MaskedNLLLoss, softIoULoss
    a = bench.bench_args(o.batch, o.imsize, o.T, o.dtype)
    a.num_classes, a.gt_maxseqlen = o.classes, o.T
    torch.manual_seed(0)
    enc, dec = FeatureExtractor(a).cuda(), RSIS(a).cuda()
    opts = list(build_optimizers(a, enc, dec))
    crits = [softIoULoss(), MaskedNLLLoss(None), MaskedBCELoss(0.5)]
    batch = synthetic_batch(1, o.batch, o.imsize, o.imsize, a.gt_maxseqlen, 12, a.num_classes, "cuda")
    t_run = steps_to_run(a, batch[3])
    if o.graph:
        gs = GraphedStep(a, enc, dec, crits, opts)
        step = lambda: gs(batch, t_run)
    else:
        step = lambda: runIter(a, enc, dec, *batch, crits, opts, mode="train", sync_losses=False, t_run=t_run, want_outs=False)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    if o.graph and gs.graph is None:
        print("RESULT nan capture failed: %s" % (gs.failed,))
        return
    t0 = time.time()
    for _ in range(o.steps):
        step()
    torch.cuda.synchronize()
    print("RESULT %.2f" % (1e3 * (time.time() - t0) / o.steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--classes", type=int, default=81)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imsize", type=int, default=256)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--rows", default="eager:fp32,graph:fp32,eager:bf16,graph:bf16")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--dtype", default="fp32")
    o = ap.parse_args()
    o.tree = os.path.abspath(o.tree)
    if o.child:
        child(o)
        return
    for row in o.rows.split(","):
        mode, dtype = row.split(":")
        for _rep in range(o.repeat):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", o.tree, "--steps", str(o.steps), "--classes", str(o.classes), "--batch",
                   str(o.batch), "--imsize", str(o.imsize), "--T", str(o.T), "--dtype", dtype] + (["--graph"] if mode == "graph" else [])
            r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, capture_output=True, text=True, cwd=o.tree)
            res = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
            per_step = "runs per step" in r.stdout + r.stderr
            if r.returncode != 0 or not res:
                print("%-12s %-5s FAILED (exit %d): %s" % (mode, dtype, r.returncode, (r.stderr or r.stdout)[-300:]), flush=True)
                if r.returncode in (124, 134, 137, 139, -6, -11):
                    return 1         # a time limit or a crash: start nothing more on the device
                continue
            print("%-6s %-5s classes %-4d B %d T %d %d^2  %s ms per step   decoder: %s" % (mode, dtype, o.classes, o.batch, o.T, o.imsize, res[0].split(None, 1)[1],
                                                                                        "per step" if per_step else "sequence node"), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
