"""Inference calls (torch.no_grad(), or a ConvLSTM call that saves no gates) of the fp32 convs and of the ConvLSTM cell against FLOAT64 on
the host, op by op.  For the 3x3 / stride 1 convs such a call runs kernels of its own -- the segmented-accumulation (FLUSH) instantiations of
conv3x3_direct.hip and conv_wino.hip, the grouped gate kernel, the folded BatchNorm epilogue (BNE) -- which the training-call op tests never
launch and which test_gpu_evalfold.py only compares with each other.

Two host models of the summation order (fp32 products and fp32 additions in numpy, NOT the code under test) supply the measured-against
values: `chain` (one running sum: sources in order, channels ascending, taps row-major) and `segmented` (the same order, the running sum
moved to a second fp32 total every RSIS_ACC_FLUSH = 4 chunks of 8 channels, chunks counted on across the sources as the kernel counts them).
Bars, per output element against float64:

  * outer: 2e-6 * sqrt(K) + 1e-6 (rtol 2e-6), the project's generic fp32 bar;
  * tight (direct 3x3, tile 0-6): err_gpu <= M_TIGHT * err_segmented_host + 2e-7.  M_TIGHT = twice the worst err_gpu / err_segmented_host
    measured on the MI355X over every case and variant (NOTES.md (75) has the table); it must stay <= 4;
  * the claim of conv3x3_direct.hip: at >= 47 chunks err_gpu <= 0.5 * err_chain_host (the host models alone give 0.21 .. 0.25);
  * dispatch pinned by bits: an inference call equals the training call of the same variant exactly where no segment boundary is crossed
    (<= 4 chunks) or no segmented instantiation exists (the 512-thread variants 7-9), and differs from it everywhere else;
  * ConvLSTM: with e the tight bar of the gate pre-activations, c within 1.5 e + 5e-7 and h within 1.75 e + 5e-7 (sigmoid' <= 1/4,
    tanh' <= 1, |c_prev| <= 1, |tanh| <= 1: dc <= e/4 + e/4 + e, dh <= e/4 + dc; 5e-7: expf / tanhf / the division at a few ulp);
  * folded BatchNorm: |scale|_max * e + 1e-6, scale = gamma / sqrt(var + eps) in float64 (1e-6: the fp32 affine on outputs kept below 8)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import (ACC_FLUSH, CK, assert_close, cell64 as _cell64, f32_normal as _rng, gate_bar, host_sums as _host_sums, max_err as _err,
                     mk_args, to_tensor as _t)

pytestmark = pytest.mark.gpu

M_TIGHT = 2.63        # 2 x 1.313, the worst measured ratio (NOTES.md (75))


@pytest.fixture(autouse=True)
def _reset_tile():
    from rsis_amd import ops
    ops.FORCE_TILE[0] = 0
    yield
    ops.FORCE_TILE[0] = 0


def _chunks(segs):
    return sum((c + CK - 1) // CK for c in segs)


# ---------------------------------------------------------------- 2. plain 3x3 / stride 1, every variant
CONV_CASES = [
    # (B, [Cin segs], H, W, Cout, bias)
    (2, [32], 9, 13, 40, True),           # 4 chunks: no boundary
    (2, [33], 9, 13, 40, False),          # 5: the fifth chunk holds one channel
    (2, [20, 12], 9, 13, 40, True),       # 3 + 2: boundary inside the second source, channel tails
    (2, [16, 16, 8], 8, 8, 32, True),     # 2 + 2 + 1: three sources, 8 x 8 map (the dispatcher picks variant 6)
    (2, [72], 16, 32, 72, False),         # 9: two boundaries, Cout tail
    (1, [128], 20, 40, 24, True),         # 16: partial pixel tiles in both directions, Cout <= 32
    (2, [376], 8, 8, 40, False),          # 47 \
    (2, [384], 8, 8, 40, False),          # 48  } either side of RSIS_FLUSH_MIN_CHUNKS
    (2, [392], 8, 8, 40, True),           # 49 /
    (1, [64], 16, 64, 16, False),         # 8: the dispatcher's own choice is the 512-thread variant 8
]
# indices of CONV_CASES whose dispatcher choice (tile 0) is a 512-thread variant.  This restates pick_direct_variant() of conv3x3_direct.hip
# (variant 8 on maps >= 16 x 64 with <= 64 output rows; 6 on 8 x 8 maps; otherwise 4 / 5 at these sizes): a retuned rule fails the tile-0
# bit assertions below for that reason and this set is then what to update -- the forced tiles 1-9 pin the kernels whatever the rule.
_OWN_512 = {9}
_CONV_REF = {}


def _conv_ref(k):
    """inputs, float64 reference and the two host models of CONV_CASES[k], computed once and shared by the variants"""
    if k not in _CONV_REF:
        B, segs, H, W, Cout, has_bias = CONV_CASES[k]
        Ctot = sum(segs)
        xs = [_rng(100 + 10 * k + i, (B, c, H, W)) for i, c in enumerate(segs)]
        w = _rng(200 + k, (Cout, Ctot, 3, 3), 1.0 / np.sqrt(9 * Ctot))
        b = _rng(300 + k, (Cout,)) if has_bias else None
        ref = F.conv2d(torch.cat([_t(x) for x in xs], 1).double(), _t(w).double(), _t(b).double() if has_bias else None, padding=1)
        chain, seg = _host_sums(xs, w, b)
        _CONV_REF[k] = dict(xs=xs, w=w, b=b, ref=ref, e_chain=_err(chain, ref), e_seg=_err(seg, ref))
    return _CONV_REF[k]


@pytest.mark.parametrize("tile", list(range(10)))
@pytest.mark.parametrize("k", list(range(len(CONV_CASES))), ids=["%dch" % _chunks(c[1]) + "_" + "+".join(map(str, c[1])) for c in CONV_CASES])
def test_conv3x3_inference_call(k, tile):
    from rsis_amd import ops
    B, segs, H, W, Cout, has_bias = CONV_CASES[k]
    r = _conv_ref(k)
    nq, K = _chunks(segs), 9 * sum(segs)
    ops.FORCE_TILE[0] = tile
    xd = [_t(x).cuda() for x in r["xs"]]
    wd = _t(r["w"]).cuda()
    bd = _t(r["b"]).cuda() if has_bias else None
    pack = ops.PackedConv(3, segs, stride=1, pad=1)
    with torch.no_grad():
        out = ops.conv2d(xd, wd, bd, 1, 1, pack)
    torch.cuda.synchronize()
    e_gpu = _err(out, r["ref"])
    print("\nINFER-CONV %-12s chunks %2d tile %d: err gpu %.3e  host segmented %.3e  host chain %.3e  gpu/segmented %.3f  gpu/chain %.3f"
          % ("+".join(map(str, segs)), nq, tile, e_gpu, r["e_seg"], r["e_chain"], e_gpu / r["e_seg"], e_gpu / r["e_chain"]))
    assert_close("fwd (outer bar)", out, r["ref"], 2e-6 * np.sqrt(K) + 1e-6, 2e-6)
    if tile <= 6:
        assert e_gpu <= M_TIGHT * r["e_seg"] + 2e-7, "tight bar: %.3e > %.1f * %.3e + 2e-7" % (e_gpu, M_TIGHT, r["e_seg"])
        if nq >= 47:
            assert e_gpu <= 0.5 * r["e_chain"], "segmented sums must halve the chain's error: %.3e vs chain %.3e" % (e_gpu, r["e_chain"])
    if nq < 32:                                   # (deeper: the training call may split K over the grid)
        xg = [x.clone().requires_grad_() for x in xd]
        train = ops.conv2d(xg, wd, bd, 1, 1, ops.PackedConv(3, segs, stride=1, pad=1)).detach()
        torch.cuda.synchronize()
        # (tile 0: both calls go through the same pick_direct_variant() -- the training call's grid split-K, the one thing that makes it
        #  choose differently on 8 x 8 maps, needs >= 32 chunks -- so the comparison is between instantiations of one variant here too)
        block512 = tile >= 7 or (tile == 0 and k in _OWN_512)
        if nq <= ACC_FLUSH or block512:
            assert torch.equal(out, train), "no segment boundary / no segmented instantiation: the bits of the training call"
        else:
            assert not torch.equal(out, train), "%d chunks on a 256-thread variant: the segmented kernel must have run" % nq


def test_conv3x3_stride2_and_1x1_inference_calls():
    """the unsegmented inference paths against float64 at the outer bar: the 3x3 / stride 2 forward (EPI_F2) and the 1x1 GEMM at the depth
    of the trunk's last layer"""
    from rsis_amd import ops
    for B, segs, H, W, Cout, ks, stride, pad in ((2, [72], 17, 15, 40, 3, 2, 1), (2, [2048], 4, 4, 64, 1, 1, 0)):
        C = sum(segs)
        x, w = _rng(400 + ks, (B, C, H, W)), _rng(410 + ks, (Cout, C, ks, ks), 1.0 / np.sqrt(C * ks * ks))
        ref = F.conv2d(_t(x).double(), _t(w).double(), None, stride=stride, padding=pad)
        with torch.no_grad():
            out = ops.conv2d([_t(x).cuda()], _t(w).cuda(), None, stride, pad, ops.PackedConv(ks, segs, stride=stride, pad=pad))
        torch.cuda.synchronize()
        bar = 2e-6 * np.sqrt(C * ks * ks) + 1e-6
        print("\nINFER-UNSEG %dx%d / stride %d, %d channels: err gpu %.3e (outer bar %.3e)" % (ks, ks, stride, C, _err(out, ref), bar))
        assert_close("%dx%d / stride %d" % (ks, ks, stride), out, ref, bar, 2e-6)


# ---------------------------------------------------------------- 3. ConvLSTM cell
LSTM_CASES = [
    # (B, [x segs], hid, H, W)
    (2, [8], 4, 5, 7),
    (2, [16, 16], 8, 16, 16),
    (2, [6, 5], 3, 6, 5),
    (2, [64, 64], 32, 8, 8),
    (1, [128], 128, 4, 4),
    (2, [24], 16, 9, 12),
]


def _gate_bar(w, b, xs, state, gates64):
    """e: the tight bar of the gate pre-activations of this call (host segmented model of the gate conv over the sources the kernel walks)"""
    return gate_bar(w, b, xs, state, gates64, M_TIGHT)


def _lstm_weights(case, seed=1):
    B, segs, hid, H, W = case
    ctot = sum(segs) + hid
    return _rng(seed, (4 * hid, ctot, 3, 3), 1.0 / np.sqrt(9 * ctot)), _rng(seed + 1, (4 * hid,), 0.2)


def _check_cell(what, h, c, h64, c64, e):
    eh, ec = _err(h, h64), _err(c, c64)
    print("\nINFER-LSTM %s: err c %.3e (bar %.3e)  err h %.3e (bar %.3e)" % (what, ec, 1.5 * e + 5e-7, eh, 1.75 * e + 5e-7))
    assert ec <= 1.5 * e + 5e-7, "%s: c %.3e > %.3e" % (what, ec, 1.5 * e + 5e-7)
    assert eh <= 1.75 * e + 5e-7, "%s: h %.3e > %.3e" % (what, eh, 1.75 * e + 5e-7)


@pytest.mark.parametrize("tile", list(range(7)))
@pytest.mark.parametrize("case", LSTM_CASES, ids=["%s_h%d_%dx%d" % ("+".join(map(str, c[1])), c[2], c[3], c[4]) for c in LSTM_CASES])
def test_convlstm_inference_call(case, tile):
    """ConvLSTMCell.forward_multi under no_grad, zero state then recurrent (the second step fed the kernel's own h0, c0)"""
    from rsis_amd import ops
    from rsis_amd.modules.clstm import ConvLSTMCell
    B, segs, hid, H, W = case
    ops.FORCE_TILE[0] = tile
    w, b = _lstm_weights(case)
    cell = ConvLSTMCell(mk_args(), sum(segs), hid, 3, 1).cuda()
    with torch.no_grad():
        cell.Gates.weight.copy_(_t(w))
        cell.Gates.bias.copy_(_t(b))
    x0 = [_rng(30 + i, (B, c, H, W)) for i, c in enumerate(segs)]
    x1 = [_rng(40 + i, (B, c, H, W)) for i, c in enumerate(segs)]
    x0d, x1d = [_t(x).cuda() for x in x0], [_t(x).cuda() for x in x1]
    with torch.no_grad():
        h0, c0 = cell.forward_multi(x0d, None)
        h1, c1 = cell.forward_multi(x1d, [h0, c0])
    torch.cuda.synchronize()
    s0 = (h0.cpu(), c0.cpu())
    rh0, rc0, g0 = _cell64(w, b, x0, None)
    rh1, rc1, g1 = _cell64(w, b, x1, s0)
    assert float(c0.abs().max()) <= 1.0                      # (what the derivation of the bar assumes of c_prev)
    _check_cell("tile %d step 0" % tile, h0, c0, rh0, rc0, _gate_bar(w, b, x0, None, g0))
    _check_cell("tile %d step 1" % tile, h1, c1, rh1, rc1, _gate_bar(w, b, x1, s0, g1))
    # dispatch by bits: the training call of the same variant on the same inputs
    t0 = cell.forward_multi([x.clone().requires_grad_() for x in x0d], None)
    t1 = cell.forward_multi([x.clone().requires_grad_() for x in x1d], [h0, c0])
    torch.cuda.synchronize()
    for step, nq, inf, tr in ((0, _chunks(segs), (h0, c0), t0), (1, _chunks(segs + [hid]), (h1, c1), t1)):
        same = torch.equal(inf[0], tr[0].detach()) and torch.equal(inf[1], tr[1].detach())
        if nq <= ACC_FLUSH:
            assert same, "step %d, %d chunks: no segment boundary, the bits of the training call" % (step, nq)
        else:
            assert not same, "step %d, %d chunks: the segmented kernel must have run" % (step, nq)


# ---------------------------------------------------------------- 4. grouped gate launch
# (the last column restates pick_direct_variant<EPI_LSTM>() and the grouped launcher's 1 -> 6, 2 -> 4, 3 -> 5 mapping in conv3x3_direct.hip:
#  8 x 8 maps 6, <= 16 wide 4, wider with <= 32 gate rows 5.  A retuned rule shows as a bit mismatch against the forced single call.)
GROUP_JOBS = [
    # (B, [x segs], hid, H, W, the variant the group runs the job on)
    (2, [64, 64], 32, 8, 8, 6),
    (2, [16, 16], 16, 16, 16, 4),
    (2, [24], 8, 9, 40, 5),
]


def _group_setup():
    from rsis_amd import ops
    jobs = []
    for k, (B, segs, hid, H, W, variant) in enumerate(GROUP_JOBS):
        w, b = _lstm_weights((B, segs, hid, H, W), seed=60 + 2 * k)
        xs = [_rng(70 + 10 * k + i, (B, c, H, W)) for i, c in enumerate(segs)]
        rs = np.random.default_rng(80 + k)
        hp, cp = rs.uniform(-1, 1, (B, hid, H, W)).astype(np.float32), rs.uniform(-1, 1, (B, hid, H, W)).astype(np.float32)
        pack = ops.PackedConv(3, segs + [hid], lstm_hid=hid, stride=1, pad=1)
        wd, bd = _t(w).cuda(), _t(b).cuda()
        wp = pack.fwd(wd, bd)
        srcs = [_t(x).cuda() for x in xs] + [_t(hp).cuda()]
        state = (_t(hp), _t(cp))
        h64, c64, g64 = _cell64(w, b, xs, state)
        jobs.append(dict(B=B, segs=segs + [hid], hid=hid, H=H, W=W, variant=variant, pack=pack, wp=wp, keep=(wd, bd), srcs=srcs,
                         c_prev=_t(cp).cuda(), h64=h64, c64=c64, g64=g64, e=_gate_bar(w, b, xs, state, g64)))
    return jobs


def _run_group(jobs, act_of):
    """one rsis_convlstm_fwd_batch call; act_of: {job index: act_out tensor}; returns [(h, c)]"""
    from rsis_amd import _lib, ops
    from rsis_amd._lib import check, lib, stream
    arr = (_lib.LstmJob * len(jobs))()
    outs = []
    for k, (j, q) in enumerate(zip(arr, jobs)):
        h = torch.full((q["B"], q["hid"], q["H"], q["W"]), float("nan"), device="cuda")
        c = torch.full_like(h, float("nan"))
        act = act_of.get(k)
        (j.B, j.H, j.W, j.Wp, j.bias_packed, j.addend, j.c_prev, j.h_out, j.c_out, j.act_out, j.hid, j.ks, j.pad, j.tile, j.dtype, j.side_key) = (
            q["B"], q["H"], q["W"], q["wp"].data_ptr(), q["pack"].bias_p.data_ptr(), None, q["c_prev"].data_ptr(), h.data_ptr(), c.data_ptr(),
            act.data_ptr() if act is not None else None, q["hid"], 3, 1, 0, ops.DTYPE_F32, None)
        j.nsrc = len(q["srcs"])
        for i, (s, cs) in enumerate(zip(q["srcs"], q["segs"])):
            j.src[i], j.Csrc[i] = s.data_ptr(), cs
        outs.append((h, c))
    check(lib().rsis_convlstm_fwd_batch(arr, len(jobs), stream()), "rsis_convlstm_fwd_batch")
    torch.cuda.synchronize()
    return outs


def _skip_if_deterministic():
    from rsis_amd import ops
    if ops.is_deterministic():
        pytest.skip("deterministic mode issues the jobs of a group one by one: the single-call tests cover that path")


def test_grouped_gate_launch_inference():
    """three jobs without act_out in one call (variants 6, 4, 5 in one grid): each bit-equal to the single inference call forced to its
    variant, each within the ConvLSTM bar of float64"""
    from rsis_amd import ops
    from rsis_amd._lib import check, int_array, lib, ptr, ptr_array, stream
    _skip_if_deterministic()
    jobs = _group_setup()
    outs = _run_group(jobs, {})
    for k, (q, (h, c)) in enumerate(zip(jobs, outs)):
        hs, cs = torch.full_like(h, float("nan")), torch.full_like(c, float("nan"))
        check(lib().rsis_convlstm_fwd(ptr_array(q["srcs"]), int_array(q["segs"]), len(q["srcs"]), q["B"], q["H"], q["W"], ptr(q["wp"]),
                                      ptr(q["pack"].bias_p), None, ptr(q["c_prev"]), ptr(hs), ptr(cs), None, q["hid"], 3, 1, q["variant"],
                                      ops.DTYPE_F32, stream()), "rsis_convlstm_fwd")
        torch.cuda.synchronize()
        assert torch.equal(h, hs) and torch.equal(c, cs), "job %d: grouped != single inference call on variant %d" % (k, q["variant"])
        _check_cell("group job %d (%d chunks)" % (k, _chunks(q["segs"])), h, c, q["h64"], q["c64"], q["e"])


def test_grouped_gate_launch_mixed():
    """job 0 saves its gates (a training job), jobs 1-2 do not: the whole group runs the segmented kernel, job 0 still writes every gate"""
    _skip_if_deterministic()
    jobs = _group_setup()
    q = jobs[0]
    act = torch.full((q["B"], 4 * q["hid"], q["H"], q["W"]), float("nan"), device="cuda")
    outs = _run_group(jobs, {0: act})
    for k, (p, (h, c)) in enumerate(zip(jobs, outs)):
        _check_cell("mixed group job %d" % k, h, c, p["h64"], p["c64"], p["e"])
    assert not bool(torch.isnan(act).any()), "job 0 must write every saved gate"
    hid = q["hid"]
    i, f, o, g = q["g64"].chunk(4, 1)                                        # reference rows [i | f | o | g] x hid
    want = torch.stack([torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)], 2)      # (B, hid, 4, H, W): row 4 j + gate
    got = act.double().cpu().view(q["B"], hid, 4, q["H"], q["W"])
    for gate, slope in enumerate((0.25, 0.25, 0.25, 1.0)):
        eg, bar = float((got[:, :, gate] - want[:, :, gate]).abs().max()), slope * q["e"] + 5e-7
        print("\nINFER-LSTM mixed group, saved gate %d: err %.3e (bar %.3e)" % (gate, eg, bar))
        assert eg <= bar


# ---------------------------------------------------------------- 5. Winograd inference kernel
WINO_INFER_CASES = [
    # (B, Cin, Cout, H, W, bias): the <= 256-channel WINO_CASES of test_gpu_wino.py; (2, 32, 32, 5, 3): exactly one 32-channel segment
    (2, 256, 256, 16, 16, False),
    (3, 256, 256, 14, 14, False),
    (2, 64, 96, 13, 17, True),
    (1, 128, 128, 32, 64, False),
    (2, 32, 32, 5, 3, True),
    (9, 64, 64, 16, 16, False),
]


@pytest.mark.parametrize("case", WINO_INFER_CASES, ids=lambda c: "%dx%d-%d_%dx%d" % (c[0], c[1], c[2], c[3], c[4]))
def test_winograd_inference_kernel(case):
    from rsis_amd import ops
    from rsis_amd._lib import lib
    B, Cin, Cout, H, W, has_bias = case
    assert lib().rsis_conv_uses_wino(3, 1, 1, Cin, Cout, 1, 0) == 1, "not a Winograd shape: both calls would run the direct kernels"
    x, w = _rng(1, (B, Cin, H, W)), _rng(2, (Cout, Cin, 3, 3), 1.0 / np.sqrt(9 * Cin))
    b = _rng(3, (Cout,)) if has_bias else None
    ref = F.conv2d(_t(x).double(), _t(w).double(), _t(b).double() if has_bias else None, padding=1)
    xd, wd, bd = _t(x).cuda(), _t(w).cuda(), _t(b).cuda() if has_bias else None
    prev = ops.WINOGRAD_INFER[0]
    try:
        ops.WINOGRAD_INFER[0] = True
        with torch.no_grad():
            inf = ops.conv2d([xd], wd, bd, 1, 1, ops.PackedConv(3, [Cin], stride=1, pad=1, dtype=ops.DTYPE_F32_WINO))
        train = ops.conv2d([xd.clone().requires_grad_()], wd, bd, 1, 1, ops.PackedConv(3, [Cin], stride=1, pad=1, dtype=ops.DTYPE_F32_WINO)).detach()
        torch.cuda.synchronize()
    finally:
        ops.WINOGRAD_INFER[0] = prev
    e_inf, e_train = _err(inf, ref), _err(train, ref)
    print("\nINFER-WINO %r: err inference (segmented) %.3e  training call %.3e" % (case, e_inf, e_train))
    assert_close("winograd inference", inf, ref, 2e-6 * np.sqrt(9 * Cin) + 1e-6, 2e-6)
    assert e_inf <= e_train + 2e-7
    if Cin <= 32:
        assert torch.equal(inf, train), "one 32-channel segment: the bits of the training call"
    else:
        assert not torch.equal(inf, train), "%d channels: the segmented Winograd kernel must have run" % Cin


# ---------------------------------------------------------------- 6. folded BatchNorm epilogue
BN_CASES = [
    # (cin, cout, ks, H, W, bias, relu, res)
    (24, 40, 3, 20, 12, True, True, True),
    (72, 72, 3, 16, 32, False, True, False),
    (392, 40, 3, 8, 8, True, False, False),
    (64, 100, 1, 15, 15, False, True, False),
]


@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "%d-%d_k%d_%dx%d" % c[:5])
def test_folded_batchnorm_against_float64(case):
    """relu?(bn_eval(conv(x) + b) + res) in float64.  BatchNorm statistics are drawn so that |scale * conv| stays below ~3 and the output
    below 8: the fp32 affine of the epilogue (scale and shift at ~2 ulp, one fma, one add) then stays inside the bar's 1e-6."""
    from rsis_amd import ops
    cin, cout, ks, H, W, has_bias, relu, has_res = case
    B, pad, eps = 2, ks // 2, 1e-5
    rs = np.random.default_rng(500 + cin)
    x, w = _rng(510 + cin, (B, cin, H, W)), _rng(520 + cin, (cout, cin, ks, ks), 1.0 / np.sqrt(cin * ks * ks))
    b = _rng(530 + cin, (cout,), 0.2) if has_bias else None
    res = _rng(540 + cin, (B, cout, H, W), 0.5) if has_res else None
    gamma, beta = rs.uniform(0.4, 0.6, cout).astype(np.float32), rs.uniform(-0.2, 0.2, cout).astype(np.float32)
    mean, var = rs.uniform(-0.2, 0.2, cout).astype(np.float32), rs.uniform(0.8, 1.2, cout).astype(np.float32)
    conv64 = F.conv2d(_t(x).double(), _t(w).double(), _t(b).double() if has_bias else None, padding=pad)
    scale = _t(gamma).double() / torch.sqrt(_t(var).double() + eps)
    ref = (conv64 - _t(mean).double()[None, :, None, None]) * scale[None, :, None, None] + _t(beta).double()[None, :, None, None]
    if has_res:
        ref = ref + _t(res).double()
    if relu:
        ref = ref.clamp_min(0.0)
    assert float(ref.abs().max()) < 8.0
    if ks == 3:
        _chain, seg = _host_sums([x], w, b)
        e = M_TIGHT * _err(seg, conv64) + 2e-7
    else:
        e = 2e-6 * np.sqrt(cin) + 1e-6
    dev = lambda a: _t(a).cuda() if a is not None else None
    with torch.no_grad():
        out = ops.conv2d_bn_eval(dev(x), dev(w), dev(b), 1, pad, ops.PackedConv(ks, [cin], stride=1, pad=pad), dev(gamma), dev(beta), dev(mean), dev(var), eps,
                                 relu=relu, res=dev(res))
    assert out is not None, "no folded epilogue for this conv: the case list names only covered ones"
    torch.cuda.synchronize()
    bar = float(scale.abs().max()) * e + 1e-6
    print("\nINFER-BN %r: err %.3e (bar %.3e)" % (case, _err(out, ref), bar))
    assert_close("folded conv + BatchNorm", out, ref, bar)
