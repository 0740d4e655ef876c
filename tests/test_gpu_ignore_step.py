"""The training step with an ignore map (runIter(..., ignore=), GraphedStep on 6-tuples): imsize 64, batch 2, -maxseqlen 3 -gt_maxseqlen 4,
the library's deterministic mode (so that "equal" can mean bit-equal).
  * the IoU loss runIter returns agrees with a float64 restatement computed here from the returned logits, assignment and map;
  * an all-zero map is the step without a map, bit for bit (losses and every parameter after one update);
  * a map over pixels the predictions touch changes the update;
  * GraphedStep: the first replay equals an eager step from the same state, and a SECOND batch with another map, replayed through the same
    capture, equals its eager step -- the map is a live static input, not a constant of the capture; the same once under -dtype bf16;
  * the torch.bmm fallback (taken where the kernels refuse the shapes) states the same definition: loss against float64, a zero gradient
    under the map, its one line on stderr."""
import copy

import numpy as np
import pytest
import torch

import loss_path_cases as L
import softiou_ignore_cases as C
from helpers import mk_args

pytestmark = pytest.mark.gpu
B, S, T, GT, HIDDEN = 2, 64, 3, 4, 32


@pytest.fixture
def deterministic():
    from rsis_amd import ops
    prev = ops.set_deterministic(True)
    yield
    ops.set_deterministic(prev)


def _setup(dtype="fp32"):
    from rsis_amd.modules import FeatureExtractor, RSIS
    from rsis_amd.synthetic import synthetic_batch
    from rsis_amd.train import steps_to_run
    from rsis_amd.utils.objectives import MaskedBCELoss, MaskedNLLLoss, softIoULoss
    a = mk_args(hidden_size=HIDDEN, maxseqlen=T, gt_maxseqlen=GT, lr=1e-3, lr_cnn=1e-6, weight_decay=1e-6, weight_decay_cnn=1e-6, optim="adam",
                optim_cnn="adam", imsize=S, batch_size=B, seed=3, dtype=dtype, ignore_regions=True)
    torch.manual_seed(0)
    enc0, dec0 = FeatureExtractor(a).cuda(), RSIS(a).cuda()
    batches = [synthetic_batch(sd, B, S, S, GT, T, a.num_classes, "cuda", ignore_regions=True) for sd in (5, 6)]
    assert all(len(b) == 6 and b[5].dtype == torch.uint8 and tuple(b[5].shape) == (B, S * S) for b in batches)
    assert not torch.equal(batches[0][5], batches[1][5]) and int(batches[0][5].sum()) > 0
    crits = [softIoULoss(), MaskedNLLLoss(None), MaskedBCELoss(a.stop_balance_weight)]
    t_run = steps_to_run(a, batches[0][3])
    assert t_run == steps_to_run(a, batches[1][3]) == T
    return a, enc0, dec0, batches, t_run, crits


def _state(opts):
    torch.cuda.synchronize()
    return {o.group.name: o.group.flat_p.detach().clone() for o in opts}


def _fresh(a, enc0, dec0):
    from rsis_amd.train import build_optimizers
    enc, dec = copy.deepcopy(enc0), copy.deepcopy(dec0)
    return enc, dec, list(build_optimizers(a, enc, dec))


def _step(a, enc, dec, opts, crits, batch, t_run, ignore, **kw):
    from rsis_amd.train import runIter
    return runIter(a, enc, dec, *batch[:5], crits, opts, mode="train", sync_losses=False, t_run=t_run, want_outs=False, ignore=ignore, **kw)


def test_iou_loss_agrees_with_float64(deterministic):
    """losses[1] (the masked mean of the matched costs, rsis_loss_tail) against float64 from the returned logits, assignment and map.
    Bar: the mean over the selected rows of the per-pair cost bar 4 E / U + 8 u (E = M_IOU_IGN * err_host of these inputs), plus the
    tail's own fp32 mean: a chain of n <= B T costs in [0, 1] and one division, (n + 1) u of the sum."""
    a, enc0, dec0, batches, t_run, crits = _setup()
    enc, dec, opts = _fresh(a, enc0, dec0)
    batch = batches[0]
    losses, outs, perms = _step(a, enc, dec, opts, crits, batch, t_run, batch[5])
    logits, perm = outs[0].float().cpu().numpy(), perms[2].cpu().numpy()
    y, ign, sw = batch[1].cpu().numpy(), batch[5].cpu().numpy(), batch[3].cpu().numpy()[:, :t_run]
    S64 = C.sums64_ignore(L.sigmoid64(logits), y, ign)
    err_host = float(np.abs(C.sums_chain32_ignore(logits, y, ign).astype(np.float64) - S64).max())
    cost, den = L.cost64(S64)                                              # (B, G, T)
    bi, ti = np.arange(B)[:, None], np.arange(t_run)[None, :]
    gi = perm[:, :t_run]
    sel = sw > 0
    n = int(sel.sum())
    assert n > 0
    want = float(cost[bi, gi, ti][sel].sum() / n)
    bar = float((4 * C.M_IOU_IGN * err_host / den[bi, gi, ti] + 8 * L.U24)[sel].sum() / n) + (n + 1) * L.U24 * max(1.0, want)
    got = float(losses[1])
    print("iou loss %.9f, float64 %.9f, |diff| %.3e, bar %.3e" % (got, want, abs(got - want), bar))
    assert abs(got - want) <= bar
    # the map matters to this number: the unmasked restatement is elsewhere
    cost0, _ = L.cost64(L.sums64(L.sigmoid64(logits), y))
    assert abs(float(cost0[bi, gi, ti][sel].sum() / n) - want) > 100 * bar


def test_zero_map_is_the_step_without_a_map(deterministic):
    a, enc0, dec0, batches, t_run, crits = _setup()
    batch = batches[0]
    res = []
    for ignore in (None, torch.zeros_like(batch[5])):
        enc, dec, opts = _fresh(a, enc0, dec0)
        losses, _o, _p = _step(a, enc, dec, opts, crits, batch, t_run, ignore)
        res.append((torch.stack(list(losses)).clone(), _state(opts)))
    (l0, p0), (l1, p1) = res
    assert torch.equal(l0, l1), (l0, l1)
    assert all(torch.equal(p0[k], p1[k]) for k in p0)


def test_map_changes_the_update(deterministic):
    a, enc0, dec0, batches, t_run, crits = _setup()
    batch = batches[0]
    res = []
    for ignore in (None, batch[5]):
        enc, dec, opts = _fresh(a, enc0, dec0)
        _step(a, enc, dec, opts, crits, batch, t_run, ignore)
        res.append(_state(opts))
    assert not torch.equal(res[0]["dec"], res[1]["dec"])


def _graph_against_eager(dtype):
    """2 warm-up steps on batch 0, then batch 0 again and batch 0 under ANOTHER map: eager, against GraphedStep (capture + first replay,
    then a replay of the same capture with the other map copied into its static input)"""
    from rsis_amd.train import GraphedStep
    a, enc0, dec0, batches, t_run, crits = _setup(dtype)
    other = tuple(batches[0][:5]) + (batches[1][5],)            # the same five tensors, another map: only the map differs
    seq = [batches[0], batches[0], batches[0], other]
    enc, dec, opts = _fresh(a, enc0, dec0)
    eager = []
    for b in seq:
        _step(a, enc, dec, opts, crits, b, t_run, b[5])
        eager.append(_state(opts))
    enc, dec, opts = _fresh(a, enc0, dec0)
    g = GraphedStep(a, enc, dec, crits, opts, None, warm=2)
    graph = []
    for b in seq:
        g(b, t_run)
        graph.append(_state(opts))
    assert g.graph is not None, "capture failed: %s" % g.failed
    assert len(g.static) == 6 and g.static[5].dtype == torch.uint8
    g.release()
    for k, (e, r) in enumerate(zip(eager, graph)):
        for name in e:
            assert torch.equal(e[name], r[name]), "step %d, %s: eager and graph differ by %.3e" % (
                k, name, float((e[name].double() - r[name].double()).abs().max()))
    # the other map did something: the state after replaying it is not the state a fourth replay of batch 0 reaches
    enc, dec, opts = _fresh(a, enc0, dec0)
    g = GraphedStep(a, enc, dec, crits, opts, None, warm=2)
    for b in (batches[0],) * 4:
        g(b, t_run)
    same_map = _state(opts)
    assert g.graph is not None, "capture failed: %s" % g.failed
    g.release()
    assert torch.equal(same_map["dec"], eager[2]["dec"]) is False             # (it moved on from step 3)
    assert not torch.equal(same_map["dec"], graph[3]["dec"])


def test_graphed_step_takes_the_map_as_a_live_input(deterministic):
    _graph_against_eager("fp32")


def test_graphed_step_takes_the_map_as_a_live_input_bf16(deterministic):
    """the loss kernels are fp32 under both conv dtypes: eager-against-graph equality only"""
    _graph_against_eager("bf16")


def test_bmm_fallback_with_a_map(deterministic, monkeypatch, capfd):
    """runIter on its torch.bmm path with a map.  The path is taken where ops.softiou_supported says no (N % 8 != 0, more than 128
    predictions or slots); here that answer is forced at the step's own shapes, so that the fused step is at hand to compare with.
      * the IoU loss against the float64 restatement.  Bar: any fp32 summation of N non-negative terms is within (N - 1) u of its sum,
        the fp32 sigmoid and product add 5 u: E <= (N + 4) u per sum, so 4 E / U <= 4 (N + 4) u per cost, + 8 u, + the mean's (n + 1) u;
      * the `keep` rows handed to the loss are the map, one row per (image, prediction);
      * d loss / d logits is zero under the map and not zero elsewhere;
      * "softiou-bmm" is announced once."""
    from rsis_amd import ops, train
    from rsis_amd.utils import hungarian
    a, enc0, dec0, batches, t_run, crits = _setup()
    batch = batches[0]
    N = S * S
    monkeypatch.setattr(ops, "softiou_supported", lambda *_a: False)
    train._LOGGED.discard("softiou-bmm")
    seen = {}
    real = hungarian.softIoU

    def spy(target, out, e=1e-6, keep=None):
        seen["keep"] = keep
        out.register_hook(lambda grad: seen.__setitem__("grad", grad.detach().clone()))
        return real(target, out, e, keep=keep)
    monkeypatch.setattr(hungarian, "softIoU", spy)
    enc, dec, opts = _fresh(a, enc0, dec0)
    losses, outs, perms = _step(a, enc, dec, opts, crits, batch, t_run, batch[5])
    torch.cuda.synchronize()
    assert capfd.readouterr().err.count("soft-IoU scores through torch.bmm") == 1
    kept = (batch[5] == 0)
    assert tuple(seen["keep"].shape) == (B * t_run, N)
    assert torch.equal(seen["keep"].reshape(B, t_run, N) > 0, kept.unsqueeze(1).expand(-1, t_run, -1))
    grad = seen["grad"].reshape(B, t_run, N)
    under = (~kept).unsqueeze(1).expand_as(grad)
    assert float(grad[under].abs().max()) == 0.0 and float(grad[~under].abs().max()) > 0.0
    logits, perm = outs[0].float().cpu().numpy(), perms[2].cpu().numpy()
    y, ign, sw = batch[1].cpu().numpy(), batch[5].cpu().numpy(), batch[3].cpu().numpy()[:, :t_run]
    cost, _den = L.cost64(C.sums64_ignore(L.sigmoid64(logits), y, ign))
    bi, ti = np.arange(B)[:, None], np.arange(t_run)[None, :]
    sel = sw > 0
    n = int(sel.sum())
    want = float(cost[bi, perm[:, :t_run], ti][sel].sum() / n)
    bar = (4 * (N + 4) + 8 + n + 1) * L.U24
    got = float(losses[1])
    print("bmm fallback: iou loss %.9f, float64 %.9f, |diff| %.3e, bar %.3e" % (got, want, abs(got - want), bar))
    assert abs(got - want) <= bar
    # and the fused step from the same state agrees with it within the same bar plus its own (test_iou_loss_agrees_with_float64)
    monkeypatch.undo()
    enc, dec, opts = _fresh(a, enc0, dec0)
    fused, _o, _p = _step(a, enc, dec, opts, crits, batch, t_run, batch[5])
    assert abs(float(fused[1]) - got) <= 2 * bar
