"""`-skip_mode sum | mul | none` on the one-node sequence decoder (rsis_amd/decoder_seq.py) and the kernels `mul` adds
(csrc/pointwise.hip, csrc/blk_dec.hip).

  kernels     fp32: rsis_upsample_bilinear_ac_mul_fwd EQUAL to the unscaled entry point's output times m on one case per launch path
              (skip_mode_cases.MUL_FWD), and within the unscaled kernel's a-priori bar times |m| plus one rounding of float64;
              rsis_upsample_mul_bwd_prep: dy * m and dy * u bit for bit, u the unscaled kernel's output, and fmaf(dy, u, dm) in call order.
              blk: the same three statements on blk tensors (one bf16 rounding of y and of dy * m, an fp32 accumulator dm)
  decoder     the three modes through forward_sequence_stacked against the float64 oracle on the same weights: fp32 within the bars of
              the per-step test of these modes (test_gpu_modules.py), blk bf16 within 1.5 x the distance of the fp32-storage path + 1 %
  routing     node against the per-step path; train.py eager against --graph"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_cases as R
import skip_mode_cases as S
from helpers import assert_close, mk_args
from test_gpu_blk import HALF_ULP, _bf16, from_blk, to_blk
from test_gpu_dropout import _loss, _oracle_run, _state
from test_gpu_resample import Guarded, both_modes, dev, within_bar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_MODES = ("sum", "mul", "none")


def _abi():
    from rsis_amd import _lib
    return _lib


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ======================================================================================================================
# fp32 kernels
# ======================================================================================================================
@pytest.mark.parametrize("c", S.MUL_FWD, ids=R.case_id)
def test_mul_upsample_fwd_is_the_unscaled_output_times_m(c):
    A = _abi()
    L = A.lib()
    r = R.up_fwd_refs(c)
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    m, _ = S.mul_operands(c, 0)
    x, md = dev(r["x"]), dev(m)

    def run():
        y, u = Guarded((BC, Ho, Wo)), Guarded((BC, Ho, Wo))
        A.check(L.rsis_upsample_bilinear_ac_mul_fwd(A.ptr(x), A.ptr(md), A.ptr(y.t), BC, Hi, Wi, Ho, Wo, A.stream()), "rsis_upsample_bilinear_ac_mul_fwd")
        A.check(L.rsis_upsample_bilinear_ac_fwd(A.ptr(x), A.ptr(u.t), BC, Hi, Wi, Ho, Wo, A.stream()), "rsis_upsample_bilinear_ac_fwd")
        return [y.check("y (%s)" % c["path"]), u.check("u")]

    y, u = both_modes(run, c["path"])
    want = u * torch.from_numpy(m)
    print("%s: %d of %d elements differ from unscaled x m" % (c["path"], int((y != want).sum()), y.numel()))
    assert torch.equal(_bits(y), _bits(want)), "not the unscaled entry point's output times m"
    ref, bar = S.mul_fwd_ref(c, m)
    within_bar("mul up_fwd/ref", y, ref, bar)


@pytest.mark.parametrize("c", S.MUL_PREP, ids=R.case_id)
def test_mul_bwd_prep_stores_then_accumulates_in_call_order(c):
    """store, add, add: the three steps of a T = 3 sequence.  dy_out = fl(dy * m); dm = dy0 * u, then fmaf(dy1, u, dm), then
    fmaf(dy2, u, dm) -- u the output of the unscaled forward entry point"""
    A = _abi()
    L = A.lib()
    r = R.up_fwd_refs(c)
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    m, dys = S.mul_operands(c, 3)
    x, md = dev(r["x"]), dev(m)

    def run():
        u = Guarded((BC, Ho, Wo))
        A.check(L.rsis_upsample_bilinear_ac_fwd(A.ptr(x), A.ptr(u.t), BC, Hi, Wi, Ho, Wo, A.stream()), "rsis_upsample_bilinear_ac_fwd")
        dm = Guarded((BC, Ho, Wo))
        outs = [u.check("u")]
        for k, dy in enumerate(dys):
            g = Guarded((BC, Ho, Wo), init=dy)
            A.check(L.rsis_upsample_mul_bwd_prep(A.ptr(g.t), A.ptr(x), A.ptr(md), A.ptr(dm.t), BC, Hi, Wi, Ho, Wo, int(k > 0), A.stream()),
                    "rsis_upsample_mul_bwd_prep")
            outs += [g.check("dy after call %d" % k).clone(), dm.check("dm after call %d" % k).clone()]
        return outs

    outs = both_modes(run, c["path"])
    u = outs[0].numpy()
    acc = None
    for k, dy in enumerate(dys):
        got_dy, got_dm = outs[1 + 2 * k].numpy(), outs[2 + 2 * k].numpy()
        assert np.array_equal(got_dy.view(np.uint32), (dy * m).view(np.uint32)), "call %d: dy is not fl(dy * m)" % k
        acc = dy * u if k == 0 else S.fma32(dy, u, acc)
        bad = int((got_dm.view(np.uint32) != acc.view(np.uint32)).sum())
        print("%s call %d: %d of %d elements of dm differ" % (c["path"], k, bad, acc.size))
        assert bad == 0, "call %d: dm is not %s" % (k, "dy * u" if k == 0 else "fmaf(dy, u, dm)")
    # ... and the float64 statement: three terms, each within the forward's bar of dy * resize(x), plus the roundings of the sum
    rr = R.up_fwd_refs(c)
    want = sum(d.astype(np.float64) for d in dys) * rr["ref"]
    mag = sum(np.abs(d.astype(np.float64)) for d in dys)
    within_bar("mul prep dm/ref", torch.from_numpy(acc), want, mag * (rr["bar_ref"] + 4 * R.U * (np.abs(rr["ref"]) + rr["bar_ref"])))


def test_mul_entry_points_refuse_bad_arguments():
    A = _abi()
    L = A.lib()
    x, m, y = torch.zeros(2, 4, 4, device="cuda"), torch.zeros(2, 8, 8, device="cuda"), Guarded((2, 8, 8))
    assert L.rsis_upsample_bilinear_ac_mul_fwd(A.ptr(x), None, A.ptr(y.t), 2, 4, 4, 8, 8, A.stream()) == 1
    assert L.rsis_upsample_mul_bwd_prep(A.ptr(y.t), A.ptr(x), A.ptr(m), A.ptr(m), 2, 4, 4, 8, 8, 2, A.stream()) == 1, "accumulate is 0 or 1"
    assert L.rsis_upsample_mul_bwd_prep(A.ptr(y.t), A.ptr(x), A.ptr(m), None, 2, 4, 4, 8, 8, 0, A.stream()) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all()), "a refused call wrote something"


# ======================================================================================================================
# blk kernels
# ======================================================================================================================
BLK_SHAPES = [(2, 8, 3, 5, 7, 9), (2, 16, 7, 7, 14, 14), (2, 8, 4, 4, 4, 4), (1, 16, 6, 8, 6, 8), (2, 8, 19, 25, 37, 50)]


def _blk_data(shape):
    B, Cc, Hi, Wi, Ho, Wo = shape
    torch.manual_seed(3 * Hi + Wo)
    x = _bf16(torch.randn(B, Cc, Hi, Wi, device="cuda"))
    m = _bf16(torch.randn(B, Cc, Ho, Wo, device="cuda"))
    dys = [_bf16(torch.randn(B, Cc, Ho, Wo, device="cuda")) for _ in range(3)]
    return x, m, dys


@pytest.mark.parametrize("shape", BLK_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_blk_mul_upsample_fwd(shape):
    """(odd maps, 7 -> 14 with 16 channels, the identity resize with 8 and with 16 channels, several blocks)"""
    from rsis_amd import ops
    F = torch.nn.functional
    B, Cc, Hi, Wi, Ho, Wo = shape
    x, m, _dys = _blk_data(shape)
    xb = to_blk(x)

    def mul_fwd(mm):
        y = torch.empty((B, Cc // 8, Ho, Wo, 8), dtype=torch.bfloat16, device="cuda")
        ops.blk_upsample_mul_fwd_batch([ops.blk_resize_mul_job(xb, y, to_blk(mm))])
        return y

    # m constant per channel plane (bf16 values, a zero among them): the scaled kernel with that scale
    sc = _bf16(torch.tensor([0.0, 1.0, -2.0, 0.75, 1.5, -0.3125, 3.0, 0.5], device="cuda").repeat(B * Cc // 8 + 1)[:B * Cc].view(B, Cc))
    ys = torch.empty((B, Cc // 8, Ho, Wo, 8), dtype=torch.bfloat16, device="cuda")
    ops.blk_upsample_fwd_batch([ops.blk_resize_job(xb, ys, scale=sc.contiguous())])
    yc = mul_fwd(sc.view(B, Cc, 1, 1).expand(B, Cc, Ho, Wo).contiguous())
    print("constant planes: %d cells differ from the scaled kernel" % int((_bits(yc) != _bits(ys)).sum()))
    assert torch.equal(_bits(yc), _bits(ys)), "m constant per plane: not the scaled kernel's bits"
    # a general m against float64 on the bf16-valued operands: half a bf16 ulp, and the fp32 slack of the blk resize tests
    want = F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=True) * m.double()
    assert_close("blk mul fwd", from_blk(mul_fwd(m)), want, 2e-5 * float(want.abs().max()), HALF_ULP)
    if (Hi, Wi) == (Ho, Wo):
        assert torch.equal(from_blk(mul_fwd(m)), _bf16(x * m)), "the identity resize: y = x * m with one rounding"


@pytest.mark.parametrize("shape", BLK_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_blk_mul_bwd_prep(shape):
    from rsis_amd import ops
    B, Cc, Hi, Wi, Ho, Wo = shape
    x, m, dys = _blk_data(shape)
    xb, mb = to_blk(x), to_blk(m)
    ub = torch.empty((B, Cc // 8, Ho, Wo, 8), dtype=torch.bfloat16, device="cuda")
    ops.blk_upsample_fwd_batch([ops.blk_resize_job(xb, ub)])
    u = from_blk(ub).cpu().numpy()
    dm = Guarded((B, Cc, Ho, Wo))
    acc = None
    for k, dy in enumerate(dys):
        g = to_blk(dy)
        ops.blk_upsample_mul_bwd_prep_batch([ops.blk_mul_prep_job(g, xb, mb, dm.t, k > 0)])
        assert torch.equal(from_blk(g), _bf16(dy * m)), "call %d: dy is not dy * m rounded once" % k
        d = dy.cpu().numpy()
        acc = d * u if k == 0 else S.fma32(d, u, acc)
        got = dm.check("dm after call %d" % k).cpu().numpy()
        bad = int((got.view(np.uint32) != acc.view(np.uint32)).sum())
        print("call %d: %d of %d elements of the fp32 accumulator differ" % (k, bad, acc.size))
        assert bad == 0, "call %d: dm is not %s" % (k, "dy * u" if k == 0 else "fmaf(dy, u, dm)")
    assert torch.equal(from_blk(xb), x) and torch.equal(from_blk(mb), m), "an input was written"


def test_blk_mul_jobs_of_several_levels_share_a_launch():
    """a diagonal: jobs of different shapes in one grouped launch give the bits of one launch each"""
    from rsis_amd import ops
    one, many, jobs = [], [], []
    for shape in BLK_SHAPES[:3]:
        B, Cc, Hi, Wi, Ho, Wo = shape
        x, m, _ = _blk_data(shape)
        ys = [torch.empty((B, Cc // 8, Ho, Wo, 8), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
        ops.blk_upsample_mul_fwd_batch([ops.blk_resize_mul_job(to_blk(x), ys[0], to_blk(m))])
        jobs.append(ops.blk_resize_mul_job(to_blk(x), ys[1], to_blk(m)))
        one.append(ys[0])
        many.append(ys[1])
    ops.blk_upsample_mul_fwd_batch(jobs)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(one, many))


# ======================================================================================================================
# the decoder, fp32
# ======================================================================================================================
def _models(mode, hidden, dtype="fp32", T=3, **kw):
    from oracle import filler
    from oracle import rsis_oracle as O
    from rsis_amd.modules import RSIS
    a = dict(hidden_size=hidden, maxseqlen=T, skip_mode=mode, **kw)
    odec = filler.fill_module(O.RSIS(mk_args(**a)), seed=43).double()
    dec = RSIS(mk_args(dtype=dtype, **a)).cuda()
    dec.load_state_dict({k: v.float() for k, v in odec.state_dict().items()})
    return odec, dec


def _feats(hidden, sizes, B):
    from oracle import filler
    ch = S.skip_channels(hidden)
    return [filler.tensor(43, "skipmodes.f%d" % i, (B, ch[i]) + tuple(sizes[i])) for i in range(5)]


def _node_run(dec, feats_cpu, T, gm, record=False):
    """forward + backward through forward_sequence_stacked; asserts the call ran on the sequence node"""
    from rsis_amd import decoder_seq
    feats = [f.cuda().requires_grad_() for f in feats_cpu]
    assert decoder_seq.supported(dec, feats, T) is True, "the sequence node refuses -skip_mode %s" % dec.skip_mode
    dec.zero_grad()
    was = decoder_seq.RECORD[0]
    decoder_seq.RECORD[0] = True
    try:
        decoder_seq.LAST.clear()
        res = dec.forward_sequence_stacked(feats, T)
        assert res is not None, "forward_sequence_stacked fell back to the per-step path"
        masks, probs, stops = res[:3]
        for o in (masks, probs, stops):
            assert "_DecoderSeqFn" in type(o.grad_fn).__name__
        _loss(masks, probs, stops, gm).backward()
        arg = [a.cpu() for a in decoder_seq.LAST["arg"]]
        rec = decoder_seq.LAST.get("drop")
        rec = {k: ([x.cpu() for x in v] if v is not None else None) for k, v in rec.items()} if rec else None
    finally:
        decoder_seq.RECORD[0] = was
        decoder_seq.LAST.clear()
    return dict(outs=[o.detach().cpu().double() for o in (masks, probs, stops)], dfeats=[f.grad.cpu().double() if f.grad is not None else None for f in feats],
                grads={k: p.grad.cpu().double() for k, p in dec.named_parameters()}, arg=arg, rec=rec)


def _truth(odec, feats_cpu, T, gm, B, rec=None, arg=None):
    odec.zero_grad()
    f64 = [f.double().requires_grad_() for f in feats_cpu]
    om, op, os_ = _oracle_run(odec, f64, T, rec, gm, B, arg)
    _loss(om, op, os_, gm.double()).backward()
    return dict(outs=[om.detach(), op.detach(), os_.detach()], dfeats=[f.grad for f in f64], grads={k: p.grad.clone() for k, p in odec.named_parameters()})


def _check_fp32(mode, truth, run):
    """the bars of test_gpu_modules.py::test_decoder_other_skip_modes_match_oracle"""
    for name, got, ref in zip(("masks", "class probs", "stop"), run["outs"], truth["outs"]):
        assert_close("%s.%s" % (mode, name), got, ref, 1e-4)
    for i, (got, ref) in enumerate(zip(run["dfeats"], truth["dfeats"])):
        if ref is None:                  # none: the skip features of levels 1-4 are unused
            assert mode == "none" and i >= 1 and (got is None or float(got.abs().max()) == 0.0)
            continue
        assert got is not None, "%s: no gradient for skip feature %d" % (mode, i)
        assert_close("%s.dfeat%d" % (mode, i), got, ref, 2e-4 * max(1.0, float(ref.abs().max())))
    for k, ref in truth["grads"].items():
        assert_close("%s.grad.%s" % (mode, k), run["grads"][k], ref, 2e-4 * max(1.0, float(ref.abs().max())))


FP32_CASES = [(m, p, 3) for m in NEW_MODES for p in ("pyramid", "same")] + [(m, "pyramid", 1) for m in NEW_MODES]


@pytest.mark.parametrize("mode,pyr,T", FP32_CASES, ids=["%s-%s-T%d" % c for c in FP32_CASES])
def test_decoder_fp32_on_the_node_against_the_oracle(mode, pyr, T):
    sizes = S.PYRAMID if pyr == "pyramid" else S.PYRAMID_SAME
    B = 2
    odec, dec = _models(mode, S.HS, T=T)
    feats = _feats(S.HS, sizes, B)
    from oracle import filler
    gm = filler.tensor(43, "skipmodes.gm", (B, T, 4 * sizes[-1][0] * sizes[-1][1]))
    run = _node_run(dec, feats, T, gm)
    truth = _truth(odec, feats, T, gm, B)
    if mode == "none":
        assert all(g is None for g in truth["dfeats"][1:])
    _check_fp32(mode, truth, run)


@pytest.mark.parametrize("mode", ["sum", "none"])
def test_decoder_fp32_with_dropout_on_the_recorded_scales(mode):
    """-dropout 0.5 goes through the scaled launches as it does for concat: x = s2 * up(h) (+ skip), the reference's order"""
    B, T = 2, 3
    odec, dec = _models(mode, S.HS, T=T, dropout=0.5)
    dec.__dict__["_drop_state"] = _state()
    feats = _feats(S.HS, S.PYRAMID, B)
    from oracle import filler
    gm = filler.tensor(43, "skipmodes.gm", (B, T, 4 * S.PYRAMID[-1][0] * S.PYRAMID[-1][1]))
    run = _node_run(dec, feats, T, gm)
    assert run["rec"] is not None and run["rec"]["s2"] is not None
    assert any(bool((s == 0).any()) for s in run["rec"]["s2"]) and any(bool((s > 0).any()) for s in run["rec"]["s2"])
    _check_fp32(mode, _truth(odec, feats, T, gm, B, rec=run["rec"]), run)


def test_mul_with_dropout_keeps_the_per_step_path_and_its_result():
    """supported() is False; the per-step loop on masks drawn ahead (F.dropout2d replaced in both models, call by call)"""
    from rsis_amd import decoder_seq
    F = torch.nn.functional
    B, T = 2, 3
    odec, dec = _models("mul", S.HS, T=T, dropout=0.5)
    feats_cpu = _feats(S.HS, S.PYRAMID, B)
    hs = [S.HS >> i for i in range(5)]
    gen = torch.Generator().manual_seed(11)
    scales = [[(torch.rand(B, h, generator=gen) < 0.5).double() * 2.0 for h in hs] for _t in range(T)]
    res = []
    was = F.dropout2d
    try:
        for d, fs in ((odec, [f.double().requires_grad_() for f in feats_cpu]), (dec, [f.cuda().requires_grad_() for f in feats_cpu])):
            if d is dec:
                assert decoder_seq.supported(dec, fs, T) is False and dec.forward_sequence_stacked(fs, T) is None
            calls = {"n": 0}

            def d2(x, p, training=True):
                s = scales[calls["n"] // 5][calls["n"] % 5]
                calls["n"] += 1
                return x * s.to(x.device, x.dtype).view(x.shape[0], x.shape[1], 1, 1)

            F.dropout2d = d2
            hidden, outs, loss = None, [], 0.0
            for _t in range(T):
                mk, c, s, hidden = d(fs, hidden)
                outs += [mk, c, s]
                loss = loss + mk.square().mean() + c.square().sum() + s.mean()
            loss.backward()
            assert calls["n"] == 5 * T
            res.append((outs, [f.grad for f in fs]))
    finally:
        F.dropout2d = was
    for i, (p, q) in enumerate(zip(res[0][0], res[1][0])):
        assert_close("mul+dropout.out%d" % i, q, p.detach(), 1e-4)
    for i, (p, q) in enumerate(zip(res[0][1], res[1][1])):
        assert_close("mul+dropout.dfeat%d" % i, q, p, 2e-4 * max(1.0, float(p.abs().max())))


@pytest.mark.parametrize("mode", NEW_MODES)
def test_node_against_the_per_step_path(mode):
    """same weights, training call and inference call (torch.no_grad, the way test() runs the decoder)"""
    from rsis_amd import decoder_seq
    B, T = 2, 3
    _odec, dec = _models(mode, S.HS, T=T)
    feats = [f.cuda() for f in _feats(S.HS, S.PYRAMID, B)]

    def run(node, grad):
        was = decoder_seq.ENABLED[0]
        decoder_seq.ENABLED[0] = node
        try:
            assert decoder_seq.supported(dec, feats, T) is node
            fs = [f.clone().requires_grad_(grad) for f in feats]
            with torch.enable_grad() if grad else torch.no_grad():
                outs, _hidden = dec.forward_sequence(fs, T)
            return [o.detach().clone() for step in outs for o in step]
        finally:
            decoder_seq.ENABLED[0] = was

    for grad in (True, False):
        a, b = run(True, grad), run(False, grad)
        for i, (p, q) in enumerate(zip(a, b)):
            assert_close("%s.%s.out%d" % (mode, "train" if grad else "no_grad", i), p.reshape(q.shape), q, 1e-4)


def test_none_leaves_the_unused_skip_parameters_without_a_gradient():
    """the optimizer skips parameters without a gradient (rsis_amd/optim.py): under none the node hands no gradient to skip[1..4]"""
    B, T = 2, 2
    _odec, dec = _models("none", S.HS, T=T)
    feats = [f.cuda().requires_grad_() for f in _feats(S.HS, S.PYRAMID, B)]
    masks, probs, stops = dec.forward_sequence_stacked(feats, T)[:3]
    (masks.mean() + probs.square().sum() + stops.mean()).backward()
    assert feats[0].grad is not None and float(feats[0].grad.abs().max()) > 0
    assert all(f.grad is None for f in feats[1:])


@pytest.mark.parametrize("dtype,hidden", [("fp32", 32), ("bf16", 128)], ids=["fp32", "bf16"])
def test_a_training_step_under_none_leaves_sk4_to_sk1_untouched(dtype, hidden):
    """torch.optim skips parameters without a gradient; under none sk4..sk1 / bn4..bn1 never get one (the blk trunk hands their branches
    materialised zeros): build_optimizers keeps them out of the step -- no weight decay, no moments -- while sk5 / bn5 move"""
    from rsis_amd.modules import FeatureExtractor, RSIS
    from rsis_amd.synthetic import synthetic_batch
    from rsis_amd.train import build_optimizers, runIter, steps_to_run
    from rsis_amd.utils.objectives import MaskedBCELoss, MaskedNLLLoss, softIoULoss
    a = mk_args(hidden_size=hidden, maxseqlen=3, lr=1e-3, lr_cnn=1e-5, weight_decay=1e-2, weight_decay_cnn=1e-6, optim="adam", optim_cnn="adam",
                imsize=64, batch_size=2, seed=3, skip_mode="none", dtype=dtype)
    torch.manual_seed(3)
    enc, dec = FeatureExtractor(a).cuda(), RSIS(a).cuda()
    batch = synthetic_batch(5, 2, 64, 64, a.gt_maxseqlen, 3, a.num_classes, "cuda")
    opts = list(build_optimizers(a, enc, dec))
    crits = [softIoULoss(), MaskedNLLLoss(None), MaskedBCELoss(a.stop_balance_weight)]
    names = ["sk4", "sk3", "sk2", "sk1", "bn4", "bn3", "bn2", "bn1"]
    before = {n: [p.detach().clone() for p in getattr(enc, n).parameters()] for n in names + ["sk5", "bn5"]}
    for _ in range(2):
        out = runIter(a, enc, dec, *batch, crits, opts, mode="train", sync_losses=False, t_run=steps_to_run(a, batch[3]), want_outs=False)
    assert all(np.isfinite(float(v)) for v in out[0])
    for n in names:
        for p, q in zip(getattr(enc, n).parameters(), before[n]):
            assert torch.equal(p.detach(), q), "%s moved under -skip_mode none" % n
    assert not torch.equal(enc.sk5.weight.detach(), before["sk5"][0]), "sk5 did not move"


# ======================================================================================================================
# the decoder, blk bf16
# ======================================================================================================================
@pytest.mark.parametrize("mode", NEW_MODES)
def test_decoder_blk_bf16_against_fp32_storage_and_the_oracle(mode):
    """NOTES.md (94): the comparator is the same model under RSIS_DECODER_BLK=0 (fp32 storage, bf16 operands); the blk node may be at most
    1.5 x the comparator's distance from the float64 oracle + 1 % of max |ref|, per output and per gradient (largest absolute
    difference).  The global max-pool is not continuous: each run is held to the oracle pooled at the pixels THAT run pooled, and the
    test says whether the two runs pooled the same ones."""
    from oracle import filler
    from rsis_amd import decoder_seq
    B, T = 1, 3
    odec, dec = _models(mode, S.BLK_HS, dtype="bf16", T=T)
    feats = _feats(S.BLK_HS, S.BLK_PYRAMID, B)
    gm = filler.tensor(43, "skipmodes.gm", (B, T, 4 * S.BLK_PYRAMID[-1][0] * S.BLK_PYRAMID[-1][1]))
    runs = []
    was = decoder_seq.BLK_ENABLED[0]
    try:
        for blk in (False, True):
            decoder_seq.BLK_ENABLED[0] = blk
            assert decoder_seq.blk_supported(dec, [f.cuda() for f in feats]) is blk
            runs.append(_node_run(dec, feats, T, gm))
    finally:
        decoder_seq.BLK_ENABLED[0] = was
    flips = [int((a != b).sum()) for a, b in zip(runs[0]["arg"], runs[1]["arg"])]
    same = not any(flips)
    print("%s: side max-pools that picked another pixel under blk storage, per level: %s" % (mode, flips))
    t0 = _truth(odec, feats, T, gm, B, arg=runs[0]["arg"])
    t1 = t0 if same else _truth(odec, feats, T, gm, B, arg=runs[1]["arg"])
    items = [(n, runs[0]["outs"][k], runs[1]["outs"][k], t0["outs"][k], t1["outs"][k]) for k, n in enumerate(("masks", "class probs", "stop"))]
    items += [("dfeat%d" % i, runs[0]["dfeats"][i], runs[1]["dfeats"][i], t0["dfeats"][i], t1["dfeats"][i]) for i in range(5)]
    items += [("grad." + k, runs[0]["grads"][k], runs[1]["grads"][k], t0["grads"][k], t1["grads"][k]) for k in t0["grads"]]
    worst = []
    for name, r0, r1, ref0, ref1 in items:
        if ref0 is None:
            assert mode == "none" and (r1 is None or float(r1.abs().max()) == 0.0), name
            continue
        d0, d1, top = float((r0 - ref0).abs().max()), float((r1 - ref1).abs().max()), float(ref1.abs().max())
        print("%s %-34s fp32 storage %.3e  blk %.3e  max|ref| %.3e  (blk / bar %.2f)" % (mode, name, d0, d1, top, d1 / max(1.5 * d0 + 0.01 * top, 1e-300)))
        if d1 > 1.5 * d0 + 0.01 * top:
            worst.append((name, d0, d1, top))
    assert not worst, "blk storage further from the oracle than 1.5 x fp32 storage + 1 %% of max|ref|: %s" % worst


# ======================================================================================================================
# entry points
# ======================================================================================================================
def _train(mode, extra, tmp_path, tag):
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "rsis_amd.train", "--synthetic", "--log_term", "-skip_mode", mode, "-imsize", "64",
           "-batch_size", "2", "-maxseqlen", "3", "-gt_maxseqlen", "4", "-synthetic_batches", "1", "-max_epoch", "5", "--use_class_loss",
           "--use_stop_loss", "-print_every", "1", "-models_root", str(tmp_path / ("models_" + tag)), "-model_name", "skip_" + mode] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "capture failed" not in out and "per-step-decoder" not in out and "decoder runs per step" not in out, out[-3000:]
    totals = [float(l.split("total:")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("Epoch") and "(train)" in l]
    assert len(totals) == 5 and all(np.isfinite(totals)), out[-3000:]
    return np.array(totals), out


@pytest.mark.parametrize("mode,extra", [("mul", []), ("sum", ["-dtype", "bf16"])], ids=["mul-fp32", "sum-bf16"])
def test_train_py_eager_and_graph_agree(mode, extra, tmp_path):
    """train.py on one resident synthetic batch: epochs 0-1 run eagerly, 2 captures, 3.. replay.  The bar of test_gpu_graph.py: graph
    against eager within 5 x the spread of two eager runs + 0.2 %.  Every run is a child process of its own."""
    ea, _ = _train(mode, extra, tmp_path, "a")
    eb, _ = _train(mode, extra, tmp_path, "b")
    gr, out = _train(mode, extra + ["--graph"], tmp_path, "g")
    spread = float(np.abs(ea - eb).max())
    print("%s %s: eager %s\n  graph %s\n  eager spread %.3e, graph - eager %.3e" % (mode, extra, ea, gr, spread, float(np.abs(gr - ea).max())))
    assert float(np.abs(gr - ea).max()) <= 5 * spread + 2e-3 * float(np.abs(ea).max())
