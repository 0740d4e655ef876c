"""Sequences of up to 128 predictions / ground-truth slots on the device path: the tiled soft-IoU sums (32 <= max(T, G) <= 128),
the two-columns-per-lane assignment (65 <= G <= 128), one training iteration against the torch.bmm / scipy fallbacks, and the
capture of such an iteration as a hipGraph."""
import copy

import numpy as np
import pytest
import torch

from helpers import assert_close, mk_args

pytestmark = pytest.mark.gpu

COST_TOL = (2e-6, 1e-5)       # tests/test_gpu_ops.py::test_softiou_sums_and_matched_loss


@pytest.mark.parametrize("B,T,G,N", [(2, 32, 31, 64), (2, 31, 32, 64), (1, 33, 33, 520), (2, 64, 64, 264), (2, 63, 65, 8),
                                     (1, 128, 128, 520), (2, 127, 100, 4096), (3, 10, 100, 72), (2, 40, 72, 16384)])
def test_softiou_sums_and_matched_loss_long(B, T, G, N):
    """fused soft-IoU (rsis_softiou_sums / rsis_softiou_bwd) against the oracle's softIoU (hungarian.py:62-89) on every
    pair, and against autograd of the oracle's matched loss, at shapes that need more than one 32x32 tile"""
    from rsis_amd import ops
    from oracle import rsis_oracle as O
    rng = np.random.default_rng(5)
    logits = torch.from_numpy(rng.normal(0, 2.0, (B, T, N)).astype(np.float32))
    y = torch.from_numpy((rng.random((B, G, N)) < 0.3).astype(np.float32))
    y[:, -1] = 0                                                     # an empty ground-truth slot
    S = ops.softiou_sums(logits.cuda(), y.cuda())
    assert float(S[:, -1, -1].abs().max()) == 0.0
    cost = ops.softiou_cost_matrix(S).cpu()                          # (B, G, T)
    ref = torch.stack([torch.stack([O.softIoU(y[:, g], logits[:, t]).reshape(B) for t in range(T)], 1) for g in range(G)], 1)
    assert_close("cost", cost, ref, *COST_TOL)
    # (a GT slot for every prediction: a permutation of the slots, and random slots for the predictions beyond G when T > G)
    perm = torch.stack([torch.from_numpy(np.concatenate([rng.permutation(G), rng.integers(0, G, max(0, T - G))])) for _ in range(B)]).long()
    lg = logits.clone().requires_grad_()
    ref_cost = O.softIoU(torch.gather(y, 1, perm[:, :T].unsqueeze(-1).expand(-1, -1, N)).reshape(-1, N), lg.reshape(-1, N)).reshape(B, T)
    w = torch.from_numpy(rng.normal(0, 1, (B, T)).astype(np.float32))
    (ref_cost * w).sum().backward()
    ld = logits.cuda().requires_grad_()
    got = ops.softiou_matched(ld, y.cuda(), perm.cuda(), S)
    (got * w.cuda()).sum().backward()
    assert_close("matched", got, ref_cost, *COST_TOL)
    assert_close("dlogits", ld.grad, lg.grad, 1e-6 * max(1.0, float(lg.grad.abs().max()) * 1e3), 1e-4)


def test_softiou_sums_long_deterministic_mode():
    """rsis_set_deterministic(1): every address of S has one contributor, so two calls return the same bits"""
    from rsis_amd import ops
    from rsis_amd._lib import lib
    B, T, G, N = 2, 40, 72, 16384
    rng = np.random.default_rng(6)
    logits = torch.from_numpy(rng.normal(0, 2.0, (B, T, N)).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.random((B, G, N)) < 0.3).astype(np.float32)).cuda()
    lib().rsis_set_deterministic(1)
    try:
        s1 = ops.softiou_sums(logits, y).clone()
        s2 = ops.softiou_sums(logits, y).clone()
    finally:
        lib().rsis_set_deterministic(0)
    assert torch.equal(s1, s2)
    assert_close("sum p", s1[:, :T, G], torch.sigmoid(logits.double()).sum(2), 0.0, 1e-5)
    assert_close("sum y", s1[:, T, :G], y.double().sum(2), 0.0, 1e-6)


@pytest.mark.parametrize("B,G,T", [(3, 65, 20), (2, 128, 128), (4, 100, 64), (2, 96, 1), (5, 127, 33), (2, 128, 1), (3, 65, 65)])
def test_assign_min_cost_long_matches_scipy(B, G, T):
    """device Hungarian == scipy.optimize.linear_sum_assignment on generic costs (unique optimum), 65 to 128 GT slots"""
    from scipy.optimize import linear_sum_assignment
    from rsis_amd import ops
    rng = np.random.default_rng(B * 1000 + G * 10 + T)
    scores = rng.uniform(0, 1, (B, G, T)).astype(np.float32)
    perm = ops.assign_min_cost(torch.from_numpy(scores).cuda()).cpu().numpy()
    for b in range(B):
        r, c = linear_sum_assignment(scores[b].astype(np.float64))
        want = np.zeros(G, dtype=np.int64)
        want[c] = r
        assert (perm[b] == want).all(), (b, perm[b], want)


def test_assign_min_cost_long_with_masked_ties():
    """the reference's score structure (invalid pairs = 10 -> ties among unused slots) at 100 GT slots: a set of distinct slots
    with the optimal total cost, equal to scipy's wherever the loss looks (valid predictions: matching one of them to an invalid
    slot costs at least 9 more than any valid pairing, so that block is unique)"""
    from scipy.optimize import linear_sum_assignment
    from rsis_amd import ops
    B, G, T, n_inst = 4, 100, 40, 37
    sc = np.random.default_rng(1).uniform(0, 1, (B, G, T)).astype(np.float32)
    sw = np.zeros(G, np.float32)
    sw[:n_inst] = 1
    valid = sw[None, :, None] * sw[None, None, :T]
    sc = sc * valid + (1 - valid) * 10
    perm = ops.assign_min_cost(torch.from_numpy(sc).cuda()).cpu().numpy()
    for b in range(B):
        r, c = linear_sum_assignment(sc[b].astype(np.float64))
        assert len(set(perm[b, :T].tolist())) == T
        assert abs(sc[b].astype(np.float64)[perm[b, :T], np.arange(T)].sum() - sc[b].astype(np.float64)[r, c].sum()) < 1e-4
        want = np.zeros(G, dtype=np.int64)
        want[c] = r
        assert (perm[b, :n_inst] == want[:n_inst]).all()
        assert (perm[b, T:] == 0).all()


def _models(a, seed=0):
    from rsis_amd.modules import FeatureExtractor, RSIS
    torch.manual_seed(seed)
    return FeatureExtractor(a).cuda(), RSIS(a).cuda()


def test_training_iteration_device_path_equals_fallbacks(monkeypatch):
    """72 GT slots x 36 steps: the iteration on the tiled sums + device assignment against the same iteration forced onto
    torch.bmm + the second pass over gathered masks + scipy on the host: same losses, same parameter gradients, and the device
    path announces no fallback.

    The matching is an arg-min that is defined only up to ties of the cost matrix (helpers.same_matching): with random weights
    the predicted masks of an image barely change over the steps, the optimum beats the next assignment by < 1e-6, and the
    scores of the two paths differ by one fp32 rounding (1.2e-7).  Measured on this batch: two runs of the SAME device path
    (fp32 atomics of the split sums) differ in 61 of 124 matched slots and by 8.9e-4 in the gradients, two runs of the fallback
    in 5 slots; every one of these assignments is optimal under either path's scores to 5e-7.  So the losses are compared
    between the device path and the fallback as it runs by itself; the device path's assignment must be optimal under the
    fallback's scores to helpers.same_matching's tie (1e-5); and the gradients are compared against the fallback evaluated
    under that assignment (a third run: bmm scores, second-pass loss, the assignment handed over), at the stated bar."""
    from scipy.optimize import linear_sum_assignment
    from rsis_amd import ops, train
    from rsis_amd.synthetic import synthetic_batch
    from rsis_amd.train import build_optimizers, runIter, steps_to_run
    from rsis_amd.utils.hungarian import match_indices
    from rsis_amd.utils.objectives import MaskedBCELoss, MaskedNLLLoss, softIoULoss
    a = mk_args(hidden_size=32, maxseqlen=36, gt_maxseqlen=72, lr=1e-3, lr_cnn=1e-5, weight_decay=1e-6, weight_decay_cnn=1e-6,
                optim="adam", optim_cnn="adam", imsize=64, batch_size=4, seed=3)
    batch = synthetic_batch(5, 4, 64, 64, 72, 30, a.num_classes, "cuda")
    t_run = steps_to_run(a, batch[3])
    crits = [softIoULoss(), MaskedNLLLoss(None), MaskedBCELoss(a.stop_balance_weight)]
    enc0, dec0 = _models(a)
    seen = {}

    def host_assign(scores):
        seen["scores"] = scores.detach().double().cpu().numpy()
        return torch.from_numpy(match_indices(scores)).to(scores.device)

    def run(assign):
        enc, dec = copy.deepcopy(enc0), copy.deepcopy(dec0)
        opts = list(build_optimizers(a, enc, dec))
        train._LOGGED.clear()
        with monkeypatch.context() as m:
            if assign is not None:
                m.setattr(ops, "softiou_supported", lambda out_masks, y_mask: False)
                m.setattr(ops, "assign_min_cost", assign)
            losses, _, perms = runIter(a, enc, dec, *batch, crits, opts, mode="train", sync_losses=False, t_run=t_run, want_outs=False,
                                       do_update=False)
        grads = torch.cat([p.grad.reshape(-1) for mod in (enc, dec) for p in mod.parameters() if p.grad is not None]).double().cpu()
        return torch.stack(losses).double().cpu(), grads, perms[2].clone()

    l_dev, g_dev, p_dev = run(None)
    assert "softiou-bmm" not in train._LOGGED and "host-assignment" not in train._LOGGED, train._LOGGED
    l_fb, g_fb, p_fb = run(host_assign)
    assert "softiou-bmm" in train._LOGGED
    l_fx, g_fx, p_fx = run(lambda scores: p_dev.clone())
    assert torch.equal(p_fx, p_dev)
    print("assignments equal: %s; losses device %s fallback %s fallback under the device's assignment %s; max |g| %.3e, max |dg| "
          "against the fallback %.3e, under the device's assignment %.3e"
          % (bool((p_dev == p_fb).all()), l_dev.tolist(), l_fb.tolist(), l_fx.tolist(), float(g_fb.abs().max()),
             float((g_dev - g_fb).abs().max()), float((g_dev - g_fx).abs().max())))
    assert_close("loss parts", l_dev[1:], l_fb[1:], *COST_TOL)
    assert_close("loss parts, same assignment", l_dev[1:], l_fx[1:], *COST_TOL)
    for b, sc in enumerate(seen["scores"]):                  # (B, G, maxseqlen) scores of the fallback
        cols = p_dev[b, :a.maxseqlen].cpu().numpy()
        assert len(set(cols.tolist())) == a.maxseqlen, (b, cols)
        ri, ci = linear_sum_assignment(sc)
        assert sc[cols, np.arange(a.maxseqlen)].sum() <= sc[ri, ci].sum() + 1e-5, (b, cols)
    assert g_dev.shape == g_fx.shape and float(g_fx.abs().max()) > 0
    assert_close("gradients", g_dev, g_fx, 2e-4 * max(1.0, float(g_fx.abs().max())), 1e-4)


def test_graphed_step_with_72_gt_slots():
    """an iteration with 72 GT slots has no host synchronisation (device assignment), so GraphedStep captures it"""
    from rsis_amd.synthetic import synthetic_batch
    from rsis_amd.train import GraphedStep, build_optimizers, steps_to_run
    from rsis_amd.utils.objectives import MaskedBCELoss, MaskedNLLLoss, softIoULoss
    a = mk_args(hidden_size=32, maxseqlen=6, gt_maxseqlen=72, lr=1e-3, lr_cnn=1e-5, weight_decay=1e-6, weight_decay_cnn=1e-6,
                optim="adam", optim_cnn="adam", imsize=64, batch_size=4, seed=3)
    batch = synthetic_batch(5, 4, 64, 64, a.gt_maxseqlen, 8, a.num_classes, "cuda")
    t_run = steps_to_run(a, batch[3])
    crits = [softIoULoss(), MaskedNLLLoss(None), MaskedBCELoss(a.stop_balance_weight)]
    enc, dec = _models(a)
    opts = list(build_optimizers(a, enc, dec))
    g = GraphedStep(a, enc, dec, crits, opts, None, warm=2)
    try:
        losses = []
        for _ in range(4):
            out = g(batch, t_run)
            losses.append([float(v) for v in out[0]])
        assert g.graph is not None, "capture failed: %s" % g.failed
        assert np.isfinite(np.asarray(losses)).all(), losses
    finally:
        g.release()
