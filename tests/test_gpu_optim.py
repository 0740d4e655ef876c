"""The fused flat SGD and RMSprop steps (rsis_sgd_step / rsis_rmsprop_step; -optim / -optim_cnn sgd, rmsprop: reference
utils/utils.py:78-87) against torch.optim.SGD(momentum) / torch.optim.RMSprop, through every layer: the raw C ABI over unaligned
ranges, FlatSGD / FlatRMSprop with parameters that get their first gradient late, a captured step, one training iteration, the
graphed training step and `python -m rsis_amd.train` end to end."""
import copy
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from helpers import mk_args

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat_cls(rule):
    from rsis_amd.optim import FlatRMSprop, FlatSGD
    return FlatSGD if rule == "sgd" else FlatRMSprop


def _torch_opt(rule, params, lr=1e-2, weight_decay=1e-2):
    if rule == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=0.9, weight_decay=weight_decay)
    return torch.optim.RMSprop(params, lr=lr, weight_decay=weight_decay)


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_flat_rule_matches_torch_with_gradless_parameters(rule, gscale):
    """12 steps; parameters 1 and 3 get their first gradient at steps 4 and 9 (torch skips a parameter whose grad is None: no decay,
    no state).  Odd sizes, so that the merged ranges start and end off 16-byte boundaries."""
    torch.manual_seed(1)
    shapes = [(7, 5), (11,), (3, 4, 2), (6,), (13,)]
    ref = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    init3 = ref[3].detach().clone()
    topt = _torch_opt(rule, ref)
    fopt = _flat_cls(rule)(mine, lr=1e-2, weight_decay=1e-2, lazy=[mine[1], mine[3]])
    fopt.gscale = gscale
    for it in range(12):
        have = [True, it >= 4, True, it >= 9, True]
        g = [torch.randn(s, device="cuda") for s in shapes]
        topt.zero_grad(set_to_none=True)
        fopt.zero_grad()
        for p, q, gi, h in zip(ref, mine, g, have):
            if h:
                p.grad = gi * gscale            # the torch side scales its gradients; the kernel folds gscale in
                q.grad.copy_(gi)
        fopt.mark_has_grad([q for q, h in zip(mine, have) if h])
        topt.step()
        fopt.step()
        for k, (p, q) in enumerate(zip(ref, mine)):
            assert float((p.detach() - q.detach()).abs().max()) < 2e-6, "param %d diverged at step %d" % (k, it)
        if it < 9:
            assert torch.equal(mine[3].detach(), init3), "an inactive parameter moved at step %d" % it
    assert fopt.group.active == [True] * 5


def _torch_formula(rule, p, g, s, lr, c0, c1, wd, gscale):
    d = g * gscale + wd * p
    if rule == "sgd":
        s = c0 * s + d
        return p - lr * s, s
    s = c0 * s + (1 - c0) * (d * d)
    return p - lr * (d / (s.sqrt() + c1)), s


@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_raw_abi_sweep_sizes_and_offsets(rule):
    """rsis_sgd_step / rsis_rmsprop_step over n in {1, 3, 4, 5, 63, 64, 65, 1000003} starting 0-3 floats into larger buffers: the
    range matches the formula evaluated by torch in fp32 on the device, and every element outside it stays bit-unchanged (a float4
    body or scalar tail that ran past the range would show here)"""
    from rsis_amd._lib import check, lib, stream
    L = lib()
    lr, wd, gscale = 1e-2, 1e-2, 0.5
    c0, c1 = (0.9, 0.0) if rule == "sgd" else (0.99, 1e-8)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for n in (1, 3, 4, 5, 63, 64, 65, 1000003):
        for off in range(4):
            tot = n + 11
            p0 = torch.randn(tot, device="cuda", generator=gen)
            g0 = torch.randn(tot, device="cuda", generator=gen)
            s0 = torch.rand(tot, device="cuda", generator=gen)
            p, g, s = p0.clone(), g0.clone(), s0.clone()
            ptr = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * off)              # noqa: E731
            if rule == "sgd":
                rc = L.rsis_sgd_step(ptr(p), ptr(g), ptr(s), n, lr, c0, wd, gscale, stream())
            else:
                rc = L.rsis_rmsprop_step(ptr(p), ptr(g), ptr(s), n, lr, c0, c1, wd, gscale, stream())
            check(rc, rule)
            torch.cuda.synchronize()
            sl = slice(off, off + n)
            want_p, want_s = _torch_formula(rule, p0[sl], g0[sl], s0[sl], lr, c0, c1, wd, gscale)
            assert float((p[sl] - want_p).abs().max()) <= 1e-6 * (1 + float(want_p.abs().max())), (n, off)
            assert float((s[sl] - want_s).abs().max()) <= 1e-6 * (1 + float(want_s.abs().max())), (n, off)
            for t, t0 in ((p, p0), (s, s0)):
                assert torch.equal(t[:off], t0[:off]) and torch.equal(t[off + n:], t0[off + n:]), (n, off)
            assert torch.equal(g, g0)
    # argument checks: NULL pointers and n < 0 are refused, n == 0 is a no-op
    x = torch.zeros(4, device="cuda")
    args = (lr, c0, wd, gscale) if rule == "sgd" else (lr, c0, c1, wd, gscale)
    fn = L.rsis_sgd_step if rule == "sgd" else L.rsis_rmsprop_step
    assert fn(None, x.data_ptr(), x.data_ptr(), 4, *args, stream()) == 1
    assert fn(x.data_ptr(), x.data_ptr(), None, 4, *args, stream()) == 1
    assert fn(x.data_ptr(), x.data_ptr(), x.data_ptr(), -1, *args, stream()) == 1
    assert fn(x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, *args, stream()) == 0


@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_captured_step_replays_like_eager_steps(rule):
    torch.manual_seed(2)
    shapes = [(33,), (5, 3), (7,)]
    a = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa = _flat_cls(rule)(a, lr=1e-2, weight_decay=1e-3, lazy=[a[2]])
    ob = _flat_cls(rule)(b, lr=1e-2, weight_decay=1e-3, lazy=[b[2]])
    grads = [torch.randn(oa.group.flat_g.numel(), device="cuda") for _ in range(5)]
    for _ in range(2):                                # the buffer is not zero when the capture starts
        oa.group.flat_g.copy_(grads[0])
        ob.group.flat_g.copy_(grads[0])
        oa.step()
        ob.step()
    ob.group.begin_graph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ob.step()
    for k in range(5):
        oa.group.flat_g.copy_(grads[k])
        ob.group.flat_g.copy_(grads[k])
        oa.step()
        graph.replay()
    torch.cuda.synchronize()
    ob.group.end_graph()
    assert torch.equal(oa.group.flat_p, ob.group.flat_p) and torch.equal(oa.group.buf, ob.group.buf)
    assert torch.equal(b[2].detach(), a[2].detach())


def _train_setup(T=3, S=64, B=4, hidden=32):
    from rsis_amd.modules import FeatureExtractor, RSIS
    from rsis_amd.synthetic import synthetic_batch
    from rsis_amd.train import steps_to_run
    from rsis_amd.utils.objectives import MaskedBCELoss, MaskedNLLLoss, softIoULoss
    a = mk_args(hidden_size=hidden, maxseqlen=T, lr=1e-3, lr_cnn=1e-4, weight_decay=1e-4, weight_decay_cnn=1e-4, optim="sgd",
                optim_cnn="rmsprop", momentum=0.9, imsize=S, batch_size=B, seed=3, use_stop_loss=False, update_encoder=True)
    torch.manual_seed(0)
    enc0, dec0 = FeatureExtractor(a).cuda(), RSIS(a).cuda()
    batch = synthetic_batch(5, B, S, S, a.gt_maxseqlen, T + 1, a.num_classes, "cuda")
    crits = [softIoULoss(), MaskedNLLLoss(None), MaskedBCELoss(a.stop_balance_weight)]
    return a, enc0, dec0, batch, steps_to_run(a, batch[3]), crits


@pytest.fixture
def deterministic():
    from rsis_amd import ops
    prev = ops.set_deterministic(True)
    yield
    ops.set_deterministic(prev)


def test_training_update_matches_torch_optim(deterministic):
    """-optim sgd -optim_cnn rmsprop --update_encoder: two iterations of runIter(do_update=False) + apply_update against
    torch.optim.SGD (decoder group) and torch.optim.RMSprop (trunk group) applied to the same flat gradients, per parameter (the stop
    head, whose loss is off, has no gradient: torch skips it and so must the flat step)"""
    from rsis_amd.train import apply_update, build_optimizers, runIter
    a, enc0, dec0, batch, t_run, crits = _train_setup()
    enc, dec = copy.deepcopy(enc0), copy.deepcopy(dec0)
    opts = list(build_optimizers(a, enc, dec))
    enc_opt, dec_opt = opts
    twins = []
    for o, rule, lr, wd in ((dec_opt, "sgd", a.lr, a.weight_decay), (enc_opt, "rmsprop", a.lr_cnn, a.weight_decay_cnn)):
        g = o.group
        tp = [torch.nn.Parameter(g.flat_p[off:off + n].clone()) for off, n in g.offsets]
        twins.append((g, tp, _torch_opt(rule, tp, lr=lr, weight_decay=wd)))
    stop = set(id(p) for p in dec.fc_stop.parameters())
    assert not any(act for p, act in zip(dec_opt.group.params, dec_opt.group.active) if id(p) in stop)
    for it in range(2):
        runIter(a, enc, dec, *batch, crits, opts, mode="train", sync_losses=False, t_run=t_run, want_outs=False, do_update=False)
        for g, tp, topt in twins:
            for i, (q, (off, n)) in enumerate(zip(tp, g.offsets)):
                with torch.no_grad():
                    q.copy_(g.flat_p[off:off + n])          # the same starting point: only the rules may differ
                q.grad = g.flat_g[off:off + n].clone() if g.active[i] else None
            topt.step()
        apply_update(a, opts, 1.0)
        torch.cuda.synchronize()
        for g, tp, _topt in twins:
            for i, (q, (off, n)) in enumerate(zip(tp, g.offsets)):
                err = float((g.flat_p[off:off + n] - q.detach()).abs().max())
                assert err < 2e-6, "%s parameter %d off by %.3e at iteration %d" % (g.name, i, err, it)
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(dec.fc_stop.parameters(), dec0.fc_stop.parameters()))


def test_graphed_training_step_equals_eager(deterministic):
    """GraphedStep (2 eager steps, then 3 replays) against 5 eager steps, bit for bit in deterministic mode, with -optim sgd
    -optim_cnn rmsprop --update_encoder"""
    from rsis_amd.train import GraphedStep, build_optimizers, runIter
    a, enc0, dec0, batch, t_run, crits = _train_setup()
    states = []
    for graphed in (False, True):
        enc, dec = copy.deepcopy(enc0), copy.deepcopy(dec0)
        opts = list(build_optimizers(a, enc, dec))
        g = GraphedStep(a, enc, dec, crits, opts, None, warm=2) if graphed else None
        losses = []
        for _ in range(5):
            out = g(batch, t_run) if graphed else runIter(a, enc, dec, *batch, crits, opts, mode="train", sync_losses=False,
                                                          t_run=t_run, want_outs=False)
            losses.append(torch.stack([v.detach().clone() for v in out[0]]))
        torch.cuda.synchronize()
        if graphed:
            assert g.graph is not None, "capture failed: %s" % g.failed
            g.release()
        st = {"losses": torch.stack(losses)}
        for o in opts:
            st[o.group.name + ".p"] = o.group.flat_p.clone()
            st[o.group.name + ".buf"] = o.group.buf.clone()
        states.append(st)
    eager, graph = states
    assert bool(torch.isfinite(eager["losses"]).all())
    bad = [k for k in eager if not torch.equal(eager[k], graph[k])]
    assert not bad, "graph replay differs from eager steps in %s" % bad
    assert float(eager["dec.buf"].abs().sum()) > 0 and float(eager["enc.buf"].abs().sum()) > 0


def _train_cmd(root, *extra):
    return [sys.executable, "-m", "rsis_amd.train", "--synthetic", "-synthetic_batches", "2", "-max_epoch", "2", "-batch_size", "4",
            "-imsize", "64", "-hidden_size", "32", "-maxseqlen", "3", "-optim", "sgd", "-optim_cnn", "rmsprop", "--update_encoder",
            "--graph", "--log_term", "-models_root", root, "-model_name", "rules"] + list(extra)


def test_train_end_to_end_and_resume(tmp_path):
    from rsis_amd.utils.utils import load_checkpoint
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    root = str(tmp_path)
    r = subprocess.run(_train_cmd(root), cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    totals = [float(line.split("total:")[1].split()[0]) for line in r.stdout.splitlines() if line.startswith("Epoch ") and "total:" in line]
    assert len(totals) == 4 and all(t == t and abs(t) < 1e30 for t in totals), r.stdout[-3000:]
    _e, _d, enc_o, dec_o, largs = load_checkpoint("rules", use_gpu=False, root=root)
    assert dec_o["optim"] == "sgd" and enc_o["optim"] == "rmsprop" and largs.optim == "sgd"
    assert float(dec_o["momentum_buffer"].abs().sum()) > 0 and float(enc_o["square_avg"].abs().sum()) > 0
    r2 = subprocess.run(_train_cmd(root, "--resume"), cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert "restart" not in r2.stdout, r2.stdout[-3000:]     # both groups restored their buffers from the checkpoint
