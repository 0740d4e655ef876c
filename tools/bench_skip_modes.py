#!/usr/bin/env python
"""Time the training iteration per `-skip_mode` (concat, sum, mul, none), as a replayed hipGraph (rsis_amd.train.GraphedStep), at BASELINE
configs[1] (fp32 256 x 256) and configs[2] (bf16 224 x 224), T = 10, batch 32.
    python tools/bench_skip_modes.py [--configs 1,2] [--modes sum,mul,none] [--steps 30] [--batch 32] [--T 10]
Per configuration and mode two legs, each on a fresh model from the same seed:
    seq     the one-node sequence decoder (rsis_amd/decoder_seq.py);
    cells   the same with the sequence node switched off (decoder_seq.ENABLED = False).  For sum / mul / none that is the per-step,
            per-level loop of RSIS.forward -- the only path these modes had before the node took them; for concat it is the wavefront
            schedule of decoder_fused with autograd's backward.
Prints the median step time of each leg (HIP events around single replays) and one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CONFIGS = {1: ("fp32", 256), 2: ("bf16", 224)}


def _leg(dtype, imsize, batch_size, T, mode, seq, steps):
    import bench
    from rsis_amd import decoder_seq
    from rsis_amd.modules import FeatureExtractor, RSIS
    from rsis_amd.synthetic import synthetic_batch
    from rsis_amd.train import GraphedStep, build_optimizers, steps_to_run
    from rsis_amd.utils.objectives import MaskedBCELoss, MaskedNLLLoss, softIoULoss
    a = bench.bench_args(batch_size, imsize, T, dtype)
    a.skip_mode = mode
    torch.manual_seed(a.seed)
    was = decoder_seq.ENABLED[0]
    decoder_seq.ENABLED[0] = seq
    try:
        encoder, decoder = FeatureExtractor(a).cuda(), RSIS(a).cuda()
        optims = list(build_optimizers(a, encoder, decoder))
        crits = [softIoULoss(), MaskedNLLLoss(None), MaskedBCELoss(a.stop_balance_weight)]
        batch = synthetic_batch(a.seed, batch_size, imsize, imsize, a.gt_maxseqlen, max(12, min(T, a.gt_maxseqlen)), a.num_classes, "cuda")
        t_run = steps_to_run(a, batch[3])
        gstep = GraphedStep(a, encoder, decoder, crits, optims, None, warm=2)
        for _ in range(5):                      # 2 eager steps, the capture, 2 replays
            losses = gstep(batch, t_run)[0]
        torch.cuda.synchronize()
        times = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            losses = gstep(batch, t_run)[0]
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        rec = {"ms": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3), "img_s": round(batch_size / (times[len(times) // 2] * 1e-3), 1),
               "graph": gstep.graphs is not None, "loss": round(float(losses[0]), 5)}
        if gstep.failed is not None:
            rec["capture_failed"] = str(gstep.failed)
        gstep.release()
        return rec
    finally:
        decoder_seq.ENABLED[0] = was


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--modes", default="concat,sum,mul,none")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--legs", default="seq,cells")
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skip_modes: no GPU visible (a CPU run cannot time a step)")
    out = {"device": torch.cuda.get_device_name(0), "batch": o.batch, "T": o.T}
    for c in [int(v) for v in o.configs.split(",")]:
        dtype, imsize = CONFIGS[c]
        for mode in o.modes.split(","):
            legs = {}
            for name, seq in (("seq", True), ("cells", False)):
                if name not in o.legs.split(","):
                    continue
                legs[name] = _leg(dtype, imsize, o.batch, o.T, mode, seq, o.steps)
                print("configs[%d] %s %dx%d  %-6s %-5s  %8.3f ms (min %.3f)  %7.1f img/s  graph=%s" % (c, dtype, imsize, imsize, mode, name,
                      legs[name]["ms"], legs[name]["ms_min"], legs[name]["img_s"], legs[name]["graph"]), flush=True)
                torch.cuda.empty_cache()
            out["configs[%d] %s" % (c, mode)] = legs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
