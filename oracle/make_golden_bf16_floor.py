"""Golden floors of tests/test_gpu_round2.py::test_bf16_backward_against_an_independent_bf16_evaluation -> tests/golden/bf16_floor_evalbn_96.npz.

The floor of a gradient is the relative L2 distance between the CPU oracle's gradient under torch's bf16 autocast and its fp32 gradient
(eval-mode encoder + 2 decoder steps, mask-only loss, 96x96, the test's fixture).  The bf16 autocast result depends on which oneDNN
kernels the host CPU runs (with AMX-BF16 the floor of enc.base.layer3.21.bn2.weight is 0.392, with AVX512-BF16 alone 0.187), so the
test reads the floors from this file instead of recomputing them on whatever CPU it runs on.  The stored floors are those of oneDNN's
AMX-BF16 kernels.

    python oracle/make_golden_bf16_floor.py
"""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import mk_args  # noqa: E402
from oracle import filler  # noqa: E402
from oracle import rsis_oracle as O  # noqa: E402

S, B, T = 96, 2, 2
OUT = os.path.join(ROOT, "tests", "golden", "bf16_floor_evalbn_96.npz")


def grads(e, d, xin, ctx):
    """every parameter gradient of the test's iteration (same fixture names as the test)"""
    e.eval()
    d.train()
    e.zero_grad()
    d.zero_grad()
    with ctx:
        feats = e(xin)
        hidden, loss = None, 0.0
        for t in range(T):
            m, _c, _s, hidden = d(feats, hidden)
            loss = loss + (m.float() * filler.tensor(5, "evalbn.gm%d" % t, m.shape).to(m.device)).sum()
    loss.backward()
    out = {("dec." + k): p.grad.detach().clone() for k, p in d.named_parameters() if p.grad is not None}
    out.update({("enc." + k): p.grad.detach().clone() for k, p in e.named_parameters() if p.grad is not None})
    return out


def main():
    a32 = mk_args(maxseqlen=T)
    oenc = filler.fill_module(O.FeatureExtractor(a32), seed=44)
    odec = filler.fill_module(O.RSIS(a32), seed=45)
    x = filler.tensor(5, "evalbn.x", (B, 3, S, S))
    g32 = grads(oenc, odec, x, contextlib.nullcontext())
    g16 = grads(oenc, odec, x, torch.autocast("cpu", dtype=torch.bfloat16))
    keys = sorted(k for k, v in g32.items() if float(v.abs().max()) >= 1e-12)
    floors = [float((g16[k].double() - g32[k].double()).norm() / g32[k].double().norm().clamp_min(1e-30)) for k in keys]
    np.savez_compressed(OUT, keys=np.array(keys), floors=np.array(floors, dtype=np.float64))
    print("wrote %s: %d floors, max %.4f" % (OUT, len(keys), max(floors)))


if __name__ == "__main__":
    main()
