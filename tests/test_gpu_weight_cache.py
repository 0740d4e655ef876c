"""The packed weight copies (ops.PackedConv) against the weights they copy, across hipGraph replays of the training step.

A conv's packed copy is rebuilt when its key (ops._WEIGHT_EPOCH, w._version, w.data_ptr(), dtype) changes.  A replay of a captured training
step (train.GraphedStep) changes every weight on the device and touches no part of that key: the copies in the captured repack_all() job table
are rewritten by the replay itself, every other copy -- the direct-kernel twin a Winograd trunk conv serves its no-grad calls from
(PackedConv.direct_twin, created by the first validation pass, i.e. after the capture), a captured test() (rsis_amd.test.GraphedTest) -- has to
notice from the key.  These tests train the way the reference's trainIters does (replays, then validation, then replays again: reference
src/train.py:54-197, 341-446) and compare every validation output with a CACHE-FREE recomputation: fresh modules built from the same arguments,
the trained state_dict() loaded into them.  The bar is torch.equal: inference launches no split-K kernel (test_gpu_graph.py:
test_graphed_inference_equals_eager), and the library's bit-reproducible mode is on for the validation losses, whose soft-IoU sums are
fp32 atomics by default (rsis_softiou_sums: two evaluations of the same logits can differ in the last bit of val.iou).

A copy that is NOT refreshed shows as a difference of 1e-6..1e-3 in every output after the second round of replays.  The frozen -> unfrozen
test guards the mode change of trainIters: the validation with the trunk frozen creates the twins BEFORE the second capture, so they are in
its job table and the replays refresh them."""
import random

import pytest
import torch

from helpers import mk_args

pytestmark = pytest.mark.gpu

B, S, T, HIDDEN = 4, 96, 3, 32


@pytest.fixture
def wino():
    """the default Winograd rule (layers 1-3 conv2: 28 convs with a direct twin) whatever RSIS_WINOGRAD / RSIS_WINOGRAD_INFER say"""
    from rsis_amd import ops
    prev = ops.WINOGRAD[0], ops.WINOGRAD_INFER[0]
    ops.WINOGRAD[0], ops.WINOGRAD_INFER[0] = {64, 128, 256}, False
    yield
    ops.WINOGRAD[0], ops.WINOGRAD_INFER[0] = prev


@pytest.fixture
def deterministic():
    from rsis_amd import ops
    prev = ops.set_deterministic(True)
    yield
    ops.set_deterministic(prev)


def _args(dtype="fp32", update_encoder=True):
    return mk_args(hidden_size=HIDDEN, maxseqlen=T, lr=1e-3, lr_cnn=1e-4, weight_decay=1e-6, weight_decay_cnn=1e-6, optim="adam",
                   optim_cnn="adam", imsize=S, batch_size=B, seed=3, dtype=dtype, update_encoder=update_encoder)


class _NoOptim(object):
    """what runIter(mode="val") asks of an optimizer.  The modules of a reference get no FlatAdam: building one bumps the packed-weight epoch
    (optim.FlatGroup), which would refresh every stale copy of the modules under test and hide what these tests look for."""

    def zero_grad(self):
        pass


def _models(a, optimizers=True):
    from rsis_amd.modules import FeatureExtractor, RSIS
    from rsis_amd.train import build_optimizers
    enc, dec = FeatureExtractor(a).cuda(), RSIS(a).cuda()
    return enc, dec, list(build_optimizers(a, enc, dec)) if optimizers else [_NoOptim(), _NoOptim()]


def _setup(dtype="fp32", update_encoder=True):
    from rsis_amd.synthetic import synthetic_batch
    from rsis_amd.train import steps_to_run
    from rsis_amd.utils.objectives import MaskedBCELoss, MaskedNLLLoss, softIoULoss
    a = _args(dtype, update_encoder)
    torch.manual_seed(0)
    enc, dec, opts = _models(a)
    batch = synthetic_batch(5, B, S, S, a.gt_maxseqlen, T + 1, a.num_classes, "cuda")
    val_batch = synthetic_batch(11, B, S, S, a.gt_maxseqlen, T + 1, a.num_classes, "cuda")
    images = torch.randn(B, 3, S, S, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    crits = [softIoULoss(), MaskedNLLLoss(None), MaskedBCELoss(a.stop_balance_weight)]
    return a, enc, dec, opts, crits, batch, steps_to_run(a, batch[3]), val_batch, images


def _validate(a, enc, dec, opts, crits, val_batch, images):
    """what a validation pass reads: runIter(mode="val") as trainIters calls it, and test() (reference src/test.py:16-50)"""
    from rsis_amd.test import test
    from rsis_amd.train import runIter
    losses, outs, _ = runIter(a, enc, dec, *val_batch, crits, opts, mode="val", sync_losses=False, want_outs=False)
    res = {k: v.detach().clone() for k, v in zip(("val.total", "val.iou", "val.stop", "val.class"), losses)}
    res["val.mask_logits"], res["val.class_probs"] = outs[0].clone(), outs[1].clone()
    for k, v in zip(("test.mask_logits", "test.class_probs", "test.stop_logits"), test(a, enc, dec, images, return_logits=True)):
        res[k] = v.clone()
    torch.cuda.synchronize()
    return res


def _reference(a, enc, dec, crits, val_batch, images):
    """the same validation on fresh modules holding the trained modules' state: every packed copy built from the live weights"""
    ref_enc, ref_dec, ref_opts = _models(a, optimizers=False)
    ref_enc.load_state_dict(enc.state_dict())
    ref_dec.load_state_dict(dec.state_dict())
    return _validate(a, ref_enc.eval(), ref_dec.eval(), ref_opts, crits, val_batch, images)


def _assert_equal(got, want, what):
    bad = ["%s: max |diff| %.3e" % (k, float((got[k].double() - want[k].double()).abs().max()))
           for k in want if not torch.equal(got[k], want[k])]
    assert not bad, "%s, against fresh modules with the same weights: %s" % (what, "; ".join(bad))


def _wino_convs(enc):
    from rsis_amd import ops
    from rsis_amd.modules.vision import HipConv2d
    return [m for m in enc.modules() if isinstance(m, HipConv2d) and m._pack.dtype == ops.DTYPE_F32_WINO]


def _max_change(before, after):
    return max(float((b.detach() - a.detach()).abs().max()) for b, a in zip(before, after))


@pytest.mark.parametrize("case", ["fp32", "fp32_wino_infer", "bf16"])
def test_val_after_graph_replays_sees_current_weights(wino, deterministic, case):
    """GraphedStep (warm 2): round 1 = 2 eager steps, the capture and 2 replays; round 2 = 3 replays; a validation pass after each round.
    fp32: the Winograd trunk convs validate on their direct twins, created by round 1's validation, after the capture.  fp32_wino_infer
    (no twin: no-grad calls on the Winograd copies of the job table) and bf16 (blk trunk, bf16 copies) guard the copies the replay rewrites."""
    from rsis_amd import ops
    from rsis_amd.train import GraphedStep
    if case == "fp32_wino_infer":
        ops.WINOGRAD_INFER[0] = True
    a, enc, dec, opts, crits, batch, t_run, val_batch, images = _setup("bf16" if case == "bf16" else "fp32")
    wino_convs = _wino_convs(enc)
    if case == "bf16":
        watched = [p for p in enc.base.parameters() if p.dim() == 4]
    else:
        assert len(wino_convs) >= 1, "no Winograd-packed conv: the test would not reach the twin path"
        watched = [m.weight for m in wino_convs]
    g = GraphedStep(a, enc, dec, crits, opts, None, warm=2)
    rounds, weights = [], []
    try:
        for r, n in enumerate((4, 3)):
            for _ in range(n):
                g(batch, t_run)
            torch.cuda.synchronize()
            assert g.graph is not None, "capture failed: %s" % g.failed
            weights.append([w.detach().clone() for w in watched])
            got = _validate(a, enc, dec, opts, crits, val_batch, images)
            _assert_equal(got, _reference(a, enc, dec, crits, val_batch, images), "%s, validation after round %d" % (case, r + 1))
            rounds.append(got)
            if case == "fp32":
                assert all(m._pack._twin is not None for m in wino_convs), "the no-grad calls did not run on the direct twins"
    finally:
        g.release()
    assert _max_change(weights[0], weights[1]) > 0, "the replays of round 2 did not change the watched trunk weights"
    moved = [k for k in rounds[0] if not torch.equal(rounds[0][k], rounds[1][k])]
    assert "val.mask_logits" in moved and "test.mask_logits" in moved, "round-2 validation equals round 1: %s" % moved


def test_val_after_frozen_to_unfrozen_switch(wino, deterministic):
    """trainIters' mode change (train.py: `-finetune_after`, a new capture key when update_encoder flips): a capture with the trunk frozen
    (its forward on the training-call kernels, ops.TRAINING_FORWARD) and a validation; then that capture released, update_encoder on, a new
    GraphedStep captured and replayed, and a validation again."""
    from rsis_amd.train import GraphedStep
    a, enc, dec, opts, crits, batch, t_run, val_batch, images = _setup("fp32", update_encoder=False)
    wino_convs = _wino_convs(enc)
    assert len(wino_convs) >= 1
    trunk0 = [m.weight.detach().clone() for m in wino_convs]
    g = GraphedStep(a, enc, dec, crits, opts, None, warm=2)
    try:
        for _ in range(4):
            g(batch, t_run)
        assert g.graph is not None, "capture failed (frozen trunk): %s" % g.failed
        frozen = _validate(a, enc, dec, opts, crits, val_batch, images)
        _assert_equal(frozen, _reference(a, enc, dec, crits, val_batch, images), "validation with the trunk frozen")
        assert _max_change(trunk0, [m.weight for m in wino_convs]) == 0, "the frozen trunk moved"
    finally:
        g.release()
    a.update_encoder = True
    g = GraphedStep(a, enc, dec, crits, opts, None, warm=2)
    try:
        for _ in range(6):
            g(batch, t_run)
        assert g.graph is not None, "capture failed (trunk training): %s" % g.failed
        torch.cuda.synchronize()
        got = _validate(a, enc, dec, opts, crits, val_batch, images)
        _assert_equal(got, _reference(a, enc, dec, crits, val_batch, images), "validation after the switch to update_encoder")
    finally:
        g.release()
    assert all(m._pack._twin is not None for m in wino_convs)
    assert _max_change(trunk0, [m.weight for m in wino_convs]) > 0, "the trunk did not train after the switch"
    assert not torch.equal(frozen["test.mask_logits"], got["test.mask_logits"])


def test_trainiters_graph_val_losses_match_eager(tmp_path, monkeypatch, wino, deterministic):
    """trainIters on --synthetic data, 3 epochs from the same seed, `--graph` against eager: every validation loss of every epoch within 1e-6
    relative (deterministic mode: replayed training == eager training, test_gpu_determinism.py claim 2).  4 training batches of one capture
    key per epoch (both synthetic batches stop at t = maxseqlen), so the key is captured in epoch 0 -- 2 eager steps, the capture -- and every
    later training step is a replay; the default -finetune_after 0 trains the trunk from epoch 0."""
    from rsis_amd import train as T_
    from rsis_amd.args import get_parser
    orig = T_.runIter

    def run(graph):
        events = []

        def spy(*args, **kw):
            capturing = torch.cuda.is_current_stream_capturing()
            out = orig(*args, **kw)
            if kw.get("mode") == "val":
                events.append(("val", torch.stack([v.detach() for v in out[0]]).double().cpu()))
            elif capturing:
                events.append(("capture", None))
            return out

        monkeypatch.setattr(T_, "runIter", spy)
        name = "graph" if graph else "eager"
        argv = ["--synthetic", "-synthetic_batches", "4", "-batch_size", str(B), "-imsize", str(S), "-maxseqlen", str(T), "-hidden_size",
                str(HIDDEN), "-lr", "1e-3", "-lr_cnn", "1e-4", "-finetune_after", "0", "-max_epoch", "3", "-seed", "3", "-model_name", name,
                "-models_root", str(tmp_path / name), "--log_term"] + (["--graph"] if graph else [])
        args = get_parser().parse_args(argv)
        torch.manual_seed(args.seed)
        random.seed(args.seed)
        torch.cuda.manual_seed(args.seed)
        T_.trainIters(args)
        torch.cuda.synchronize()
        monkeypatch.setattr(T_, "runIter", orig)
        return events

    ev_graph, ev_eager = run(True), run(False)
    kinds = [k for k, _ in ev_graph]
    assert kinds.count("capture") == 1 and kinds.index("capture") < kinds.index("val"), \
        "expected ONE capture, before the first validation: %s" % kinds
    assert "capture" not in [k for k, _ in ev_eager]
    vg = torch.stack([v for k, v in ev_graph if k == "val"])
    ve = torch.stack([v for k, v in ev_eager if k == "val"])
    assert vg.shape == ve.shape == (3, 4), (vg.shape, ve.shape)
    rel = (vg - ve).abs() / ve.abs().clamp_min(1e-30)
    assert float(rel.max()) <= 1e-6, "validation losses [total, iou, stop, class] per epoch, --graph vs eager (max rel %.3e):\n%s\n%s" \
        % (float(rel.max()), vg.numpy(), ve.numpy())
    moved = float(((ve[1:, 0] - ve[:-1, 0]).abs() / ve[:-1, 0].abs()).min())
    assert moved > 1e-4, "validation loss barely moved between epochs (%.3e): the comparison has no power" % moved


def test_graphed_test_recaptures_after_weight_change(wino, deterministic):
    """rsis_amd.test.GraphedTest past its capture, then the weights change twice -- one eager FlatAdam step with a non-zero gradient, then a
    load_state_dict of other weights: the next call after each change returns what test() on fresh modules with those weights returns."""
    from rsis_amd.test import GraphedTest, test
    a = _args()
    torch.manual_seed(0)
    enc, dec, opts = _models(a)
    x = torch.randn(B, 3, S, S, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    names = ("mask_logits", "class_probs", "stop_logits")

    def reference():
        ref_enc, ref_dec, _ = _models(a, optimizers=False)
        ref_enc.load_state_dict(enc.state_dict())
        ref_dec.load_state_dict(dec.state_dict())
        out = dict(zip(names, [t.clone() for t in test(a, ref_enc, ref_dec, x, return_logits=True)]))
        torch.cuda.synchronize()
        return out

    g = GraphedTest(a, enc, dec, return_logits=True, warm=1)
    for _ in range(3):
        before = dict(zip(names, [t.clone() for t in g(x)]))
    assert g.graph is not None
    _assert_equal(before, reference(), "GraphedTest before any weight change")

    def check(what, prev):
        """the next call and the two after it (the capture with the new weights and a replay of it) against the reference"""
        want = reference()
        for k in range(3):
            got = dict(zip(names, [t.clone() for t in g(x)]))
            _assert_equal(got, want, "GraphedTest, call %d after %s" % (k + 1, what))
        assert g.graph is not None
        assert not torch.equal(got["mask_logits"], prev["mask_logits"]), "%s changed nothing" % what
        return got

    gen = torch.Generator("cuda").manual_seed(1)
    for o in opts:                                     # change 1: one eager Adam step of both groups
        o.zero_grad()
        o.group.flat_g.copy_(torch.randn(o.group.flat_g.shape, device="cuda", generator=gen))
        o.step()
    got = check("an eager optimizer step", before)

    torch.manual_seed(1)                               # change 2: other weights through load_state_dict
    other_enc, other_dec, _ = _models(a, optimizers=False)
    enc.load_state_dict(other_enc.state_dict())
    dec.load_state_dict(other_dec.state_dict())
    check("load_state_dict", got)
