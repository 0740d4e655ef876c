"""The wide class / stop heads (rsis_heads_wide_fwd / rsis_heads_wide_bwd, csrc/losses.hip) against FLOAT64 through the C ABI, and the
paths they open: the one-node sequence decoder at 81 classes, at batches above 64 and at a batch of one.  Cases and the a priori bounds:
heads_wide_cases.py (checked by test_heads_wide_host.py); builders, references and the guarded-buffer harness: loss_path_cases.py /
test_gpu_loss_path.py.

  EXACT  : integer data, probs 1 / 2^k -- the stop logit, d side and every parameter gradient on top of an integer prefill EQUAL float64.
  NORMAL : seeded Gaussian data (`hot`: a saturated softmax) within the bounds derived in heads_wide_cases.py; nothing is fitted.
Every output is a guarded view, checked after each call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import heads_wide_cases as W
import loss_path_cases as L
from helpers import Guarded, assert_close, mk_args, to_tensor as _t
from test_gpu_loss_path import GuardedInt, HeadsBwd, _abi, _dev, run_heads_fwd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, UNSUPPORTED = 0, 1, 3
U24 = L.U24
_DATA = {}


def _cached(key, build):
    if key not in _DATA:
        _DATA[key] = build()
    return _DATA[key]


def _exact(s):
    return _cached(("exact", L.heads_id(s)), lambda: L.heads_exact_data(s))


def _ids(shapes):
    return [pytest.param(s, id=L.heads_id(s)) for s in shapes]


def wide_fwd(sides, Wc, bc, Ws, bs, rows=None, ncls=None, Cs=None):
    """rsis_heads_wide_fwd without keys on guarded outputs; returns (status, probs, stop) -- the Guarded objects"""
    A = _abi()
    rows = sides[0].shape[0] if rows is None else rows
    ncls = Wc.shape[0] if ncls is None else ncls
    Cs = [s.shape[1] for s in sides] if Cs is None else Cs
    probs, stop = Guarded((max(rows, 1), Wc.shape[0])), Guarded((max(rows, 1),))
    rc = A.lib().rsis_heads_wide_fwd(None, None, None, A.ptr_array(sides), A.int_array(Cs), len(Cs), rows, A.ptr(Wc), A.ptr(bc), ncls, A.ptr(Ws),
                                     A.ptr(bs), A.ptr(probs.t), A.ptr(stop.t), A.stream())
    torch.cuda.synchronize()
    probs.check("probs"), stop.check("stop")
    return rc, probs, stop


class WideBwd(HeadsBwd):
    """test_gpu_loss_path.HeadsBwd on rsis_heads_wide_bwd: the same operands, guards and comparisons, plus a guarded scratch"""

    def call(self, rows=None, ncls=None, Cs=None, scratch_floats=None):
        A = _abi()
        rows = self.rows if rows is None else rows
        ncls = self.ncls if ncls is None else ncls
        Cs = self.Cs if Cs is None else Cs
        need = max(rows, 1) * (self.ncls + 1)
        self.scratch = Guarded((need if scratch_floats is None else max(scratch_floats, 1),))
        po = lambda name, t: None if name in self.null else A.ptr(t)
        dsides = [None if "dside%d" % i in self.null else g.t for i, g in enumerate(self.dside)]
        rc = A.lib().rsis_heads_wide_bwd(A.ptr_array(self.sides), A.int_array(Cs), len(Cs), rows, A.ptr(self.Wc), ncls, A.ptr(self.Ws), A.ptr(self.probs),
                                         po("dprobs", self.dprobs), po("dstop", self.dstop), A.ptr_array(dsides), po("dWc", self.par["dWc"].t),
                                         po("dbc", self.par["dbc"].t), po("dWs", self.par["dWs"].t), po("dbs", self.par["dbs"].t), A.ptr(self.scratch.t),
                                         need if scratch_floats is None else scratch_floats, A.stream())
        torch.cuda.synchronize()
        for i, g in enumerate(self.dside):
            g.check("dside[%d]" % i)
        for k, g in self.par.items():
            g.check(k)
        self.scratch.check("scratch")
        return rc

    def untouched(self):
        """no output byte was written: d side and the scratch at their sentinel, the parameter gradients at their fill"""
        return (all(g.untouched() for g in self.dside) and self.scratch.untouched() and
                all(np.array_equal(g.t.cpu().numpy(), self.fill[k]) for k, g in self.par.items()))


# ======================================================================================================================
# exact
# ======================================================================================================================
@pytest.mark.parametrize("s", _ids(W.EXACT_SHAPES))
def test_wide_fwd_stop_exact(s):
    """integer features and weights: the stop logit EQUALS float64; the class probabilities are a distribution"""
    d = _exact(s)
    rc, probs, stop = wide_fwd([_dev(a) for a in d["sides"]], _dev(d["Wc"]), _dev(d["bc"]), _dev(d["Ws"]), _dev(d["bs"]))
    assert rc == OK
    assert_close("stop, exact", stop.t, d["stop"], 0.0)
    p = probs.t.double().cpu()
    assert bool((p >= 0).all()) and float((p.sum(1) - 1).abs().max()) <= (s[2] + 8) * U24


@pytest.mark.parametrize("s", _ids(W.EXACT_SHAPES))
def test_wide_bwd_exact_and_reproducible(s):
    """d side and every gradient on top of its integer prefill EQUAL float64; a second call on fresh buffers gives the same bits"""
    d = _exact(s)
    h, h2 = WideBwd(d, d["fill"]), WideBwd(d, d["fill"])
    assert h.call() == OK and h2.call() == OK
    h.compare(d["ref"], "exact")
    for a, b in zip(h.dside + list(h.par.values()), h2.dside + list(h2.par.values())):
        assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32))
    dl = np.concatenate([d["ref"]["dl"], d["dstop"].astype(np.float64)[:, None]], 1)
    assert_close("scratch: the d-logits", h.scratch.t.view(s[0], s[2] + 1), dl, 0.0)


@pytest.mark.parametrize("null", [("dprobs",), ("dstop",), ("dside1",), ("dWc",), ("dWs",), ("dbc", "dbs"), ("dWc", "dbc", "dWs", "dbs"),
                                  ("dside0", "dside1", "dside2", "dside3", "dside4")], ids=lambda n: "+".join(n) if len(n) < 3 else n[0] + "..")
def test_wide_bwd_null_pointers(null):
    """the NULL semantics of rsis_heads_bwd: a NULL gradient input counts as zero, a NULL output is skipped, the rest EQUALS float64"""
    d = _exact(W.NULL_SHAPE)
    ref = L.heads_bwd64(d["sides"], d["Wc"], d["Ws"], d["probs"], None if "dprobs" in null else d["dprobs"], None if "dstop" in null else d["dstop"])
    h = WideBwd(d, d["fill"], null)
    assert h.call() == OK
    h.compare(ref, "null " + "+".join(null))


def test_wide_bwd_accumulates_over_calls():
    """two calls into the same parameter buffers: fill + 2 x the gradient (still exact: 2 x 37 rows stay far below 2^24)"""
    d = _exact(W.NULL_SHAPE)
    h = WideBwd(d, d["fill"])
    assert h.call() == OK and h.call() == OK
    twice = {k: (2 * v if k != "dside" else v) for k, v in d["ref"].items()}
    h.compare(twice, "two calls")


def test_wide_fwd_keys_equals_wide_fwd_on_decoded_values():
    """rsis_heads_wide_fwd with keys on loss_path_cases.keys_data(): side_out has the BITS of the value, arg_out the pixel, and probs /
    stop the bits the call without keys gives on the decoded features"""
    A = _abi()
    d = L.keys_data()
    rows, Cs, ncls = L.KEYS_SHAPE
    keys = [_t(k.view(np.int64)).cuda() for k in d["keys"]]
    side_out, arg_out = [Guarded((rows, c)) for c in Cs], [GuardedInt((rows, c), torch.int32) for c in Cs]
    probs, stop = Guarded((rows, ncls)), Guarded((rows,))
    Wc, bc, Ws, bs = (_dev(d[k]) for k in ("Wc", "bc", "Ws", "bs"))
    A.check(A.lib().rsis_heads_wide_fwd(A.ptr_array(keys), A.ptr_array([g.t for g in side_out]), A.ptr_array([g.t for g in arg_out]), None, A.int_array(Cs),
                                        len(Cs), rows, A.ptr(Wc), A.ptr(bc), ncls, A.ptr(Ws), A.ptr(bs), A.ptr(probs.t), A.ptr(stop.t), A.stream()),
            "rsis_heads_wide_fwd(keys)")
    torch.cuda.synchronize()
    for i, (so, ao) in enumerate(zip(side_out, arg_out)):
        so.check("side_out[%d]" % i), ao.check("arg_out[%d]" % i)
        assert np.array_equal(so.t.cpu().numpy().view(np.uint32), d["vals"][i].view(np.uint32)), "side_out[%d]: not the bits of the value" % i
        assert np.array_equal(ao.t.cpu().numpy(), d["pix"][i]), "arg_out[%d]" % i
    probs.check("probs"), stop.check("stop")
    rc, p2, s2 = wide_fwd([_dev(v) for v in d["vals"]], Wc, bc, Ws, bs)
    assert rc == OK
    assert torch.equal(probs.t.view(torch.int32), p2.t.view(torch.int32)) and torch.equal(stop.t.view(torch.int32), s2.t.view(torch.int32))
    assert bool(torch.isfinite(probs.t).all()) and bool(torch.isfinite(stop.t).all())


# ======================================================================================================================
# refusals
# ======================================================================================================================
@pytest.mark.parametrize("what", ["ncls_1025", "k_2049", "rows_0", "short_scratch"])
def test_wide_refusals_write_nothing(what):
    """beyond the limits: RSIS_ERR_UNSUPPORTED; a scratch one float short: RSIS_ERR_ARG; every guarded output still holds its fill.
    (The buffers are those of a valid case; the refused call only CLAIMS the larger shape, so nothing would be read out of bounds either.)"""
    d = _exact((9, [2048], 256))
    sides = [_dev(a) for a in d["sides"]]
    Wc, bc, Ws, bs = _dev(d["Wc"]), _dev(d["bc"]), _dev(d["Ws"]), _dev(d["bs"])
    kw = dict(ncls_1025=dict(ncls=1025), k_2049=dict(Cs=[2049]), rows_0=dict(rows=0), short_scratch=dict(scratch_floats=9 * 257 - 1))[what]
    want = ERR_ARG if what == "short_scratch" else UNSUPPORTED
    if what != "short_scratch":
        rc, probs, stop = wide_fwd(sides, Wc, bc, Ws, bs, **kw)
        assert rc == want and probs.untouched() and stop.untouched()
    h = WideBwd(d, d["fill"])
    assert h.call(**kw) == want
    assert h.untouched(), "a refused call wrote an output"


# ======================================================================================================================
# normal data: a priori bounds
# ======================================================================================================================
def _within(what, got, ref, bound):
    err = np.abs(got.detach().double().cpu().numpy().reshape(np.shape(ref)) - ref)
    worst = float((err / bound).max())
    print("%-28s worst err / bound %.4f  (max err %.3e)" % (what, worst, float(err.max())))
    assert (err <= bound).all(), "%s: %.3e over its bound at %s" % (what, float((err - bound).max()), np.unravel_index((err - bound).argmax(), err.shape))


def _check_normal(s, regime, fwd):
    d = _cached(("normal", L.heads_id(s), regime), lambda: L.heads_normal_data(s, regime))
    pb, sb = W.fwd_bounds(d)
    rc, probs, stop = fwd([_dev(a) for a in d["sides"]], _dev(d["Wc"]), _dev(d["bc"]), _dev(d["Ws"]), _dev(d["bs"]))
    assert rc == OK
    _within("probs", probs.t, d["probs"], pb)
    _within("stop", stop.t, d["stop"], sb)
    h = WideBwd(d)
    assert h.call() == OK
    b, ref = W.bwd_bounds(d), d["ref"]
    _within("dside", torch.cat([g.t for g in h.dside], 1), ref["dside"], b["dside"])
    for k in ("dWc", "dbc", "dWs", "dbs"):
        _within(k, h.par[k].t, ref[k], b[k])


@pytest.mark.parametrize("regime", ["normal", "hot"])
@pytest.mark.parametrize("s", _ids(W.NORMAL_SHAPES))
def test_wide_normal(s, regime):
    """probs, stop, d side and the parameter gradients within the a priori bounds of heads_wide_cases.py of float64"""
    _check_normal(s, regime, wide_fwd)


@pytest.mark.parametrize("regime", ["normal", "hot"])
def test_wide_agrees_with_small_where_both_accept(regime):
    """(64, [2048], 64): both families take the call; the wide results lie within the same a priori bounds of float64, and so do the small
    family's forward results -- bit equality is not required (ops.heads_family never swaps them)"""
    s = W.BOTH_SHAPE
    assert L.heads_fits(s[0], sum(s[1]), s[2])
    _check_normal(s, regime, wide_fwd)
    d = _DATA[("normal", L.heads_id(s), regime)]
    pb, sb = W.fwd_bounds(d)
    p, st = run_heads_fwd([_dev(a) for a in d["sides"]], _dev(d["Wc"]), _dev(d["bc"]), _dev(d["Ws"]), _dev(d["bs"]))
    _within("probs (small)", p, d["probs"], pb)
    _within("stop (small)", st, d["stop"], sb)


# ======================================================================================================================
# module level
# ======================================================================================================================
def _feats(seed, B, hs, top, grad=True):
    from oracle import filler
    chans = [hs, hs, hs // 2, hs // 4, hs // 8]
    fs = [filler.tensor(seed, "hw.f%d" % i, (B, chans[i], top << i, top << i)).cuda() for i in range(5)]
    return [f.requires_grad_() for f in fs] if grad else fs


def _run_decoder(dec, feats, T, seq):
    """(class probs (B, T, C), stop (B, T, 1), masks (B, T, N)) and the parameter gradients, on the sequence node or per step"""
    from oracle import filler
    from rsis_amd import decoder_fused, decoder_seq
    was = decoder_seq.ENABLED[0], decoder_fused.FUSED_POOL[0]
    try:
        if not seq:
            decoder_seq.ENABLED[0] = decoder_fused.FUSED_POOL[0] = False
        dec.zero_grad()
        if seq:
            st = dec.forward_sequence_stacked(feats, T)
            assert st is not None, "the sequence node refused the model"
            masks, probs, stops = st[0], st[1], st[2]
        else:
            assert dec.forward_sequence_stacked(feats, T) is None
            steps, _hid = dec.forward_sequence(feats, T)
            masks = torch.stack([m.flatten(1) for m, _c, _s in steps], 1)
            probs, stops = torch.stack([c for _m, c, _s in steps], 1), torch.stack([s for _m, _c, s in steps], 1)
        gm = filler.tensor(11, "hw.gm", tuple(masks.shape)).to(masks.device, masks.dtype)
        ((masks * gm).sum() + (probs * probs).sum() * 20 + stops.sum()).backward()
    finally:
        decoder_seq.ENABLED[0], decoder_fused.FUSED_POOL[0] = was
    return [probs.detach().clone(), stops.detach().clone(), masks.detach().clone()], {k: p.grad.clone() for k, p in dec.named_parameters()}


@pytest.mark.parametrize("ncls,B,top", [(81, 2, 2), (21, 65, 1)], ids=["81_classes_b2_im64", "21_classes_b65_im32"])
def test_sequence_node_takes_wide_heads_and_large_batches(ncls, B, top):
    """hidden 128, T = 3: the model runs on the one-node sequence decoder (forward_sequence_stacked is not None) and its outputs and every
    decoder parameter gradient agree with the per-step path to the tolerances test_gpu_modules.py holds the two paths to
    (test_wavefront_sequence_equals_per_step_loop: outputs 1e-6, gradients 1e-4 of their scale)"""
    from oracle import filler
    from rsis_amd.modules import RSIS
    T = 3
    dec = filler.fill_module(RSIS(mk_args(hidden_size=128, num_classes=ncls, maxseqlen=T)), seed=5).cuda()
    o_seq, g_seq = _run_decoder(dec, _feats(3, B, 128, top), T, True)
    o_ps, g_ps = _run_decoder(dec, _feats(3, B, 128, top), T, False)
    assert tuple(o_seq[0].shape) == (B, T, ncls) and tuple(o_seq[1].shape) == (B, T, 1)
    for name, q, p in zip(("class", "stop", "masks"), o_seq, o_ps):
        assert_close(name, q, p.reshape(q.shape), 1e-6 * max(1.0, float(p.abs().max())), 1e-6)
    for k, p in g_ps.items():
        assert_close("grad." + k, g_seq[k], p, 1e-4 * max(1.0, float(p.abs().max())), 1e-4)


def test_sequence_node_bf16_blk_hand_over_at_81_classes():
    """-dtype bf16, 81 classes: the encoder hands blk skip features over (5-D) and the decoder runs the blk sequence node; class / stop
    outputs and decoder parameter gradients against the per-step path on the same features in fp32 NCHW, to the distances
    test_gpu_blk_dec.py allows between blk and fp32 storage (outputs 2 % of their largest, gradients 6 % relative L2)"""
    from oracle import filler
    from rsis_amd import blk_trunk, decoder_seq, train as _train
    from rsis_amd.modules import FeatureExtractor, RSIS
    T = 3
    a = mk_args(hidden_size=128, num_classes=81, maxseqlen=T, dtype="bf16")
    enc = filler.fill_module(FeatureExtractor(a), seed=44).cuda().eval()
    dec = filler.fill_module(RSIS(a), seed=5).cuda()
    x = filler.tensor(2, "hw.x", (2, 3, 64, 64)).cuda()
    assert _train._blk_skips_ok(enc, dec, x, T)
    with torch.no_grad():
        feats = enc(x, blk_skips=True)
    assert any(f.dim() == 5 for f in feats) and decoder_seq.supported(dec, feats, T) and decoder_seq.blk_supported(dec, feats)
    o_seq, g_seq = _run_decoder(dec, feats, T, True)
    dense = [blk_trunk.to_nchw(f) if f.dim() == 5 else f for f in feats]
    o_ps, g_ps = _run_decoder(dec, dense, T, False)
    for name, q, p in zip(("class", "stop"), o_seq, o_ps):
        assert bool(torch.isfinite(q).all())
        assert float((q - p.reshape(q.shape)).abs().max()) <= 0.02 * float(p.abs().max()), name
    for k, p in g_ps.items():
        e = float((g_seq[k] - p).norm() / p.norm().clamp_min(1e-30))
        assert e <= 0.06, "grad.%s: %.3f relative L2 from the per-step path" % (k, e)


def test_inference_at_batch_one():
    """test() and GraphedTest on ONE image (README's Pascal evaluation, -batch_size 1): the ordinary (1, T, H, W), (1, T, C), (1, T, 1)
    and, eval-mode BatchNorm keeping the rows independent, row 0 of a batch that holds the image twice, to 1e-5"""
    from oracle import filler
    from rsis_amd.modules import FeatureExtractor, RSIS
    from rsis_amd.test import GraphedTest, test as hip_test
    T, C = 3, 21
    a = mk_args(hidden_size=128, num_classes=C, maxseqlen=T)
    enc = filler.fill_module(FeatureExtractor(a), seed=44).cuda()
    dec = filler.fill_module(RSIS(a), seed=45).cuda()
    x = filler.tensor(4, "hw.x1", (1, 3, 64, 64)).cuda()
    two = hip_test(a, enc, dec, torch.cat([x, x], 0))
    one = hip_test(a, enc, dec, x)
    assert [tuple(t.shape) for t in one] == [(1, T, 64, 64), (1, T, C), (1, T, 1)]
    for name, p, q in zip(("masks", "classes", "stops"), one, two):
        assert_close(name, p, q[:1], 1e-5)
    g = GraphedTest(a, enc, dec, warm=1)
    for _ in range(3):                                  # eager, capture + replay, replay
        got = [t.clone() for t in g(x)]
    assert g.graph is not None
    assert [tuple(t.shape) for t in got] == [(1, T, 64, 64), (1, T, C), (1, T, 1)]
    for name, p, q in zip(("masks", "classes", "stops"), got, one):
        assert_close("graphed " + name, p, q, 1e-5)


# ======================================================================================================================
# command level
# ======================================================================================================================
@pytest.mark.parametrize("extra", [[], ["--graph", "-dtype", "bf16"]], ids=["eager_fp32", "graph_bf16"])
def test_train_py_at_81_classes_stays_on_the_sequence_node(extra, tmp_path):
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "rsis_amd.train", "--synthetic", "-num_classes", "81", "-batch_size", "2", "-maxseqlen", "3",
           "-gt_maxseqlen", "4", "-imsize", "64", "-synthetic_batches", "2", "-max_epoch", "1", "--use_class_loss", "--use_stop_loss", "--log_term",
           "-models_root", str(tmp_path / "models"), "-model_name", "wide81"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "per-step-decoder" not in r.stdout + r.stderr and "decoder runs per step" not in r.stdout + r.stderr
    assert "nan" not in r.stdout.lower() and "capture failed" not in r.stdout + r.stderr


def test_eval_py_at_batch_one(tmp_path):
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "rsis_amd.eval", "--synthetic", "-batch_size", "1", "-maxseqlen", "3", "-imsize", "64",
           "-synthetic_batches", "8", "-models_root", str(tmp_path / "models"), "-model_name", "b1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
