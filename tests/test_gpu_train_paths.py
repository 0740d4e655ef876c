"""Training calls of the fp32 convs, their data gradients and the ConvLSTM forward against FLOAT64 on the host, through the C ABI:
rsis_conv2d_fwd with tile + 100 (the training-call marker: `precise` = 0, grid split-K allowed), rsis_conv2d_dgrad, rsis_convlstm_fwd with
act_out.  These are the instantiations the inference tests never launch: EPI_PLAIN / EPI_F2 / EPI_S2 of conv3x3_direct.hip with the grid
split-K, the forward / scatter / DGRAD forms of conv_igemm.hip at every tile code, conv_c1.hip at one step.  Cases: train_paths_cases.py.

Two data regimes:

  * EXACT (coverage and indexing): inputs, weights, bias, addend and prefill are integers in -3..3 stored as fp32; sum |terms| of every
    output is below 2^24 (test_train_paths_host.py), so fp32 sums are exact in ANY order -- MFMA, K-split waves and atomics included --
    and every output must EQUAL the float64 reference, in the default and in the deterministic mode.
  * NORMAL (rounding): seeded N(0, 1) data, weights scaled by 1 / sqrt(K).  Bars per output element against float64:
      outer    2e-6 sqrt(K) + 1e-6, rtol 2e-6 (the bar of test_gpu_wino.py and test_gpu_infer_paths.py), everywhere;
      tight    err_gpu <= M * err_host + 2e-7, err_host the numpy model of the summation order (helpers.host_sums / host_sums_conv /
               host_sums_dgrad: fp32 products and additions, channels ascending, taps row-major): `chain` where the call runs the plain
               instantiation, `segmented` where a slice is >= 48 chunks long on a 256-thread variant.  M_TRAIN (direct kernels) and
               M_IGEMM are TWICE the worst err_gpu / err_host measured on the MI355X over all cases and variants (NOTES.md (82) has
               the tables) and must stay <= 4.  Split-K cases are held to the same bar: splitting only shortens chains;
      determinism   deterministic mode: two runs give equal bits; default mode: a split-K case differs from its deterministic run
               (that is how the test knows the split happened).
  * ConvLSTM training-call forward (act_out passed): with e = M * err_chain_host(gate pre-activations) + 2e-7 and the derivation of
    test_gpu_infer_paths.py (sigmoid' <= 1/4, tanh' <= 1, |c_prev| <= 1): c within 1.5 e + 5e-7, h within 1.75 e + 5e-7, the saved
    gates i, f, o within e / 4 + 5e-7 and g within e + 5e-7 (5e-7: expf / tanhf / the division at a few ulp).  Two calls per case:
    zero state, then a state drawn uniform in (-1, 1) (fixed, so that the float64 reference is shared by the variants).

Every output is a helpers.Guarded view (64 sentinel floats on each side), checked after the call.  One line per normal case is printed:
route, variant, err_gpu, err_host, ratio."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_paths_cases as T
from helpers import Guarded, assert_close, cell64, host_sums_conv, host_sums_dgrad, max_err as _err, to_tensor as _t

pytestmark = pytest.mark.gpu

M_TRAIN = 2.39       # 2 x 1.194, the worst measured ratio of the direct kernels: the stride-2 forward of the 9 x 64 map (NOTES.md (82))
M_IGEMM = 2.92       # 2 x 1.457: the in-place strided 1x1 scatter gradient, at every tile code (NOTES.md (82))


@pytest.fixture(params=["default", "deterministic"])
def mode(request):
    from rsis_amd import ops
    prev = ops.set_deterministic(request.param == "deterministic")
    yield request.param
    ops.set_deterministic(prev)


def _dev(a):
    return _t(a).cuda() if a is not None else None


_DATA = {}


def _data(kind, c, regime):
    """host inputs and float64 references of a case, computed once and shared by the variants (never modified)"""
    key = (kind, T.case_id(c), regime)
    if key not in _DATA:
        _DATA[key] = (T.fwd_data if kind == "fwd" else T.dgrad_data)(c, regime, T.case_seed(c))
    return _DATA[key]


# ---------------------------------------------------------------- the calls
def run_fwd(c, d, tile):
    """rsis_conv2d_fwd as a training call (tile + 100); returns the output (a Guarded view, already checked)"""
    from rsis_amd import ops
    from rsis_amd._lib import check, int_array, lib, ptr, ptr_array, stream
    L = lib()
    B, H, W, stride = c["B"], c["H"], c["W"], c["stride"]
    Ho, Wo = T.out_size(c)
    pack = ops.PackedConv(c["ks"], c["segs"], stride=stride, pad=c["pad"])
    wd, bd, ad = _dev(d["w"]), _dev(d["b"]), _dev(d["add"])
    wp = pack.fwd(wd)
    xs = [_dev(x) for x in d["xs"]]
    if c.get("subsample"):          # the form ops._Conv2dFn takes by default for a strided 1x1: the stride-1 GEMM on a sub-sampled copy
        sub = Guarded((B, c["segs"][0], Ho, Wo))
        check(L.rsis_subsample2d(ptr(xs[0]), ptr(sub.t), B * c["segs"][0], H, W, stride, stream()), "rsis_subsample2d")
        torch.cuda.synchronize()
        sub.check("sub-sampled copy")
        xs, H, W, stride = [sub.t], Ho, Wo, 1
    out = Guarded((B, c["cout"], Ho, Wo))
    check(L.rsis_conv2d_fwd(ptr_array(xs), int_array(c["segs"]), len(xs), B, H, W, ptr(wp), c["cout"], c["ks"], stride, c["pad"], ptr(bd), ptr(ad),
                            ptr(out.t), Ho, Wo, tile + 100, ops.DTYPE_F32, stream()), "rsis_conv2d_fwd")
    torch.cuda.synchronize()
    out.check("forward output")
    return out.t


def run_dgrad(c, d, tile):
    """rsis_conv2d_dgrad; returns the list of destinations (Guarded views, already checked)"""
    from rsis_amd import ops
    from rsis_amd._lib import check, int_array, lib, ptr, ptr_array, stream
    B, H, W = c["B"], c["H"], c["W"]
    Hy, Wy = T.out_size(c)
    pack = ops.PackedConv(c["ks"], c["segs"], stride=c["stride"], pad=c["pad"])
    wd = pack.dgrad(_dev(d["w"]))
    dy = _dev(d["dy"])
    if c.get("inplace"):
        gs = [Guarded((B, c["segs"][0], H, W), init=_t(d["add"]))]
        addend = gs[0].t
    else:
        gs = [Guarded((B, s, H, W)) for s in c["segs"]]
        addend = _dev(d["add"])
    check(lib().rsis_conv2d_dgrad(ptr(dy), B, c["cout"], Hy, Wy, ptr(wd), pack.cin, c["ks"], c["stride"], c["pad"], ptr_array([g.t for g in gs]),
                                  int_array(c["segs"]), len(gs), H, W, ptr(addend), tile, ops.DTYPE_F32, stream()), "rsis_conv2d_dgrad")
    torch.cuda.synchronize()
    for i, g in enumerate(gs):
        g.check("dx[%d]" % i)
    return [g.t for g in gs]


def _exact_fwd(c, tile):
    d = _data("fwd", c, "exact")
    assert_close("forward, tile %d, exact" % tile, run_fwd(c, d, tile), d["ref"], 0.0)


def _exact_dgrad(c, tile):
    d = _data("dgrad", c, "exact")
    for i, (dx, ref) in enumerate(zip(run_dgrad(c, d, tile), d["refs"])):
        assert_close("dx[%d], tile %d, exact" % (i, tile), dx, ref, 0.0)


def _params(cases, tiles=None):
    return [pytest.param(c, t, id="%s-t%d" % (T.case_id(c), t)) for c in cases for t in (tiles or c["tiles"])]


# ---------------------------------------------------------------- 1. exact regime
@pytest.mark.parametrize("c,tile", _params(T.DIRECT_EXACT, T.DIRECT_TILES))
def test_direct_fwd_exact(c, tile, mode):
    _exact_fwd(c, tile)


@pytest.mark.parametrize("c,tile", _params(T.DIRECT_DGRAD_EXACT, T.DIRECT_TILES))
def test_direct_dgrad_exact(c, tile, mode):
    _exact_dgrad(c, tile)


@pytest.mark.parametrize("c,tile", _params(T.SPLIT_FWD))
def test_splitk_fwd_exact(c, tile, mode):
    _exact_fwd(c, tile)


@pytest.mark.parametrize("c,tile", _params(T.SPLIT_DGRAD))
def test_splitk_dgrad_exact(c, tile, mode):
    _exact_dgrad(c, tile)


@pytest.mark.parametrize("c,tile", _params(T.S2_EXACT, T.F2_TILES))
def test_stride2_fwd_exact(c, tile, mode):
    _exact_fwd(c, tile)


@pytest.mark.parametrize("c,tile", _params([dict(c, bias=False) for c in T.S2_EXACT], T.S2_DGRAD_TILES))
def test_stride2_dgrad_exact(c, tile, mode):
    _exact_dgrad(c, tile)


@pytest.mark.parametrize("c,tile", _params(T.IGEMM_FWD_EXACT, T.IGEMM_TILES))
def test_igemm_fwd_exact(c, tile, mode):
    _exact_fwd(c, tile)


@pytest.mark.parametrize("c,tile", _params(T.IGEMM_DGRAD_EXACT, T.IGEMM_TILES))
def test_igemm_dgrad_exact(c, tile, mode):
    _exact_dgrad(c, tile)


@pytest.mark.parametrize("c", T.C1_EXACT, ids=T.case_id)
def test_conv_out_one_step_exact(c, mode):
    """conv_out (one output channel) at one step through rsis_conv2d_fwd / rsis_conv2d_dgrad: conv_c1.hip for 4 / 8 / 16 channels on maps
    with W % 4 == 0, the MFMA path for the neighbours"""
    _exact_fwd(c, 0)
    _exact_dgrad(dict(c, bias=False), 0)


def _nst_child():
    """runs in a child process with RSIS_GEMM_NST set (the library reads it once): the two exact 1x1 cases on the LDS-DMA path at the trunk's
    64 x 64 x 32 tile (code 15, and 0: the dispatcher's choice for a 1x1 with more than 32 rows)"""
    for tile in (15, 0):
        _exact_fwd([c for c in T.IGEMM_FWD_EXACT if c.get("nst")][0], tile)
        _exact_dgrad([c for c in T.IGEMM_DGRAD_EXACT if c.get("nst")][0], tile)
    print("nst child ok: RSIS_GEMM_NST=%s" % os.environ.get("RSIS_GEMM_NST"))


@pytest.mark.parametrize("nst", [3, 4])
def test_gemm_ring_depth_exact(nst):
    """RSIS_GEMM_NST = 3 | 4, the ring depth of the trunk's 1x1 GEMM: 5 K-tiles (more than either ring holds) and 3 (fewer than depth 4)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_train_paths as t; t._nst_child()" % (here, os.path.dirname(here))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RSIS_GEMM_NST=str(nst)), timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    print(out[-2000:])
    assert r.returncode == 0, "child with RSIS_GEMM_NST=%d ended with status %d:\n%s" % (nst, r.returncode, out[-2000:])
    assert "nst child ok: RSIS_GEMM_NST=%d" % nst in out


# ---------------------------------------------------------------- 2. normal regime
_MODEL = {}


def _host_model(kind, c):
    """(err_chain, err_segmented) of the host models against float64 (max over the outputs the tight bar is taken over), once per case"""
    key = (kind, T.case_id(c))
    if key not in _MODEL:
        d = _data(kind, c, "normal")
        n = min(c["B"], T.TIGHT_IMAGES)
        if kind == "fwd":
            chain, seg = host_sums_conv([x[:n] for x in d["xs"]], d["w"], d["b"], c["stride"], c["pad"])
            ref = d["ref"][:n]
        else:
            chain, seg = host_sums_dgrad(d["dy"][:n], d["w"], c["stride"], c["pad"], c["H"], c["W"])
            ref = torch.cat(d["refs"], 1)[:n]
        if d["add"] is not None:
            chain, seg = chain + d["add"][:n], seg + d["add"][:n]
        _MODEL[key] = (_err(chain, ref), _err(seg, ref))
    return _MODEL[key]


def _normal(kind, c, tile, route, m, split=False):
    from rsis_amd import ops
    d = _data(kind, c, "normal")
    n = min(c["B"], T.TIGHT_IMAGES)
    K = (sum(c["segs"]) if kind == "fwd" else c["cout"]) * c["ks"] ** 2
    e_chain, e_seg = _host_model(kind, c)
    nq = T.chunks(c["segs"]) if kind == "fwd" else T.cdiv(c["cout"], T.CK)

    def call():
        if kind == "fwd":
            return run_fwd(c, d, tile).clone(), d["ref"]
        return torch.cat(run_dgrad(c, d, tile), 1), torch.cat(d["refs"], 1)

    def bars(what, out, ref, segmented):
        e_host = e_seg if segmented else e_chain
        e_gpu = _err(out[:n], ref[:n])
        print("\nTRAIN %-14s %-34s variant %2d %-13s: err gpu %.3e  host %s %.3e  ratio %.3f"
              % (route, T.case_id(c), tile, what, e_gpu, "segmented" if segmented else "chain", e_host, e_gpu / e_host))
        assert_close("%s (outer bar)" % what, out, ref, 2e-6 * np.sqrt(K) + 1e-6, 2e-6)
        if m is not None:
            assert e_gpu <= m * e_host + 2e-7, "%s tight bar: %.3e > %.2f * %.3e + 2e-7" % (what, e_gpu, m, e_host)

    prev = ops.set_deterministic(False)
    try:
        out, ref = call()
        # (only the split-K cases are deep enough for the segmented instantiation; a 512-thread variant has none)
        _variant, ksplit, _slices, seg_default = T.split_plan(c, tile, kind == "dgrad") if split else (tile, 1, [nq], False)
        assert split or nq < T.FLUSH_MIN_CHUNKS
        bars("default", out, ref, seg_default)
        ops.set_deterministic(True)
        det1, _ = call()
        det2, _ = call()
        seg_det = split and T.split_plan(c, tile, kind == "dgrad", deterministic=True)[3]
        bars("deterministic", det1, ref, seg_det)
        assert torch.equal(det1, det2), "deterministic mode: two runs differ"
        if split:
            if ksplit > 1:
                assert not torch.equal(out, det1), "default mode: %d K slices summed with atomics must differ from the unsplit run" % ksplit
            else:
                assert torch.equal(out, det1), "this variant makes >= 160 blocks and is not split: the bits of the deterministic run"
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("c,tile", _params(T.DIRECT_NORMAL, T.DIRECT_TILES))
def test_direct_fwd_normal(c, tile):
    _normal("fwd", c, tile, "direct fwd", M_TRAIN)


@pytest.mark.parametrize("c,tile", _params([dict(c, bias=False) for c in T.DIRECT_NORMAL], T.DIRECT_TILES))
def test_direct_dgrad_normal(c, tile):
    _normal("dgrad", c, tile, "direct dgrad", M_TRAIN)


@pytest.mark.parametrize("c,tile", _params(T.SPLIT_NORMAL))
def test_splitk_fwd_normal(c, tile):
    _normal("fwd", c, tile, "direct fwd sk", M_TRAIN, split=True)


@pytest.mark.parametrize("c,tile", _params(T.SPLIT_DGRAD_NORMAL))
def test_splitk_dgrad_normal(c, tile):
    _normal("dgrad", c, tile, "direct dgrad sk", M_TRAIN, split=True)


@pytest.mark.parametrize("c,tile", _params(T.S2_NORMAL, T.F2_TILES))
def test_stride2_fwd_normal(c, tile):
    _normal("fwd", c, tile, "direct F2", M_TRAIN)


@pytest.mark.parametrize("c,tile", _params([dict(c, bias=False) for c in T.S2_NORMAL], T.S2_DGRAD_TILES))
def test_stride2_dgrad_normal(c, tile):
    _normal("dgrad", c, tile, "direct S2", M_TRAIN)


@pytest.mark.parametrize("c,tile", _params(T.IGEMM_FWD_NORMAL, T.IGEMM_TILES))
def test_igemm_fwd_normal(c, tile):
    _normal("fwd", c, tile, "igemm fwd", M_IGEMM)


@pytest.mark.parametrize("c,tile", _params(T.IGEMM_DGRAD_NORMAL, T.IGEMM_TILES))
def test_igemm_dgrad_normal(c, tile):
    _normal("dgrad", c, tile, "igemm dgrad", M_IGEMM)


@pytest.mark.parametrize("c", [T.C1_EXACT[1]], ids=T.case_id)
def test_conv_out_one_step_normal(c):
    """conv_c1.hip forms its sums with fma on the vector ALUs (no model of that order here): the outer bar, and equal bits run to run"""
    _normal("fwd", c, 0, "c1 fwd", None)
    _normal("dgrad", dict(c, bias=False), 0, "c1 dgrad", None)


# ---------------------------------------------------------------- 3. ConvLSTM training-call forward
_LSTM = {}


def _lstm_ref(case, ks):
    """inputs, float64 cell and the chain error of the gate pre-activations of the two calls of a case, once per (case, kernel size)"""
    key = (case[0], tuple(case[1])) + tuple(case[2:]) + (ks,)
    if key not in _LSTM:
        B, segs, hid, H, W = case
        ctot, pad = sum(segs) + hid, ks // 2
        seed = 9000 + 31 * (sum(segs) + 7 * hid + 3 * H + W) + ks
        w, b = T.normal(seed, (4 * hid, ctot, ks, ks), 1.0 / np.sqrt(ks * ks * ctot)), T.normal(seed + 1, (4 * hid,), 0.2)
        rs = np.random.default_rng(seed + 2)
        state = (_t(rs.uniform(-1, 1, (B, hid, H, W)).astype(np.float32)), _t(rs.uniform(-1, 1, (B, hid, H, W)).astype(np.float32)))
        steps = []
        for k, st in enumerate((None, state)):
            xs = [T.normal(seed + 10 * (k + 1) + i, (B, c, H, W)) for i, c in enumerate(segs)]
            h64, c64, g64 = cell64(w, b, xs, st, pad=pad)
            srcs = xs + ([st[0].numpy()] if st is not None else [])
            cin = sum(s.shape[1] for s in srcs)
            chain, _seg = host_sums_conv(srcs, np.ascontiguousarray(w[:, :cin]), b, 1, pad)
            i, f, o, g = g64.chunk(4, 1)
            act64 = torch.stack([torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)], 2)      # (B, hid, 4, H, W): row 4 j + gate
            steps.append(dict(xs=xs, state=st, h64=h64, c64=c64, act64=act64, e_chain=_err(chain, g64)))
        _LSTM[key] = dict(w=w, b=b, steps=steps)
    return _LSTM[key]


def _lstm(case, ks, tile, m):
    from rsis_amd import ops
    from rsis_amd._lib import check, int_array, lib, ptr, ptr_array, stream
    B, segs, hid, H, W = case
    assert T.chunks(segs + [hid]) < T.FLUSH_MIN_CHUNKS            # (a training call below 48 chunks: the plain instantiation, `chain`)
    r = _lstm_ref(case, ks)
    pack = ops.PackedConv(ks, segs + [hid], lstm_hid=hid, stride=1, pad=ks // 2)
    wd, bd = _dev(r["w"]), _dev(r["b"])
    wp = pack.fwd(wd, bd)
    for k, s in enumerate(r["steps"]):
        srcs = [_dev(x) for x in s["xs"]] + ([s["state"][0].cuda()] if s["state"] is not None else [])
        cp = s["state"][1].cuda() if s["state"] is not None else None
        h, c, act = Guarded((B, hid, H, W)), Guarded((B, hid, H, W)), Guarded((B, 4 * hid, H, W))
        check(lib().rsis_convlstm_fwd(ptr_array(srcs), int_array([t.shape[1] for t in srcs]), len(srcs), B, H, W, ptr(wp), ptr(pack.bias_p), None,
                                      ptr(cp), ptr(h.t), ptr(c.t), ptr(act.t), hid, ks, ks // 2, tile, ops.DTYPE_F32, stream()), "rsis_convlstm_fwd")
        torch.cuda.synchronize()
        for g, what in ((h, "h"), (c, "c"), (act, "act_out")):
            g.check(what)
        e = m * s["e_chain"] + 2e-7
        ec, eh = _err(c.t, s["c64"]), _err(h.t, s["h64"])
        got = act.t.double().cpu().view(B, hid, 4, H, W)
        eg = [float((got[:, :, q] - s["act64"][:, :, q]).abs().max()) for q in range(4)]
        print("\nTRAIN-LSTM %dx%d %r tile %d step %d: e %.3e  err c %.3e  h %.3e  gates i %.3e f %.3e o %.3e g %.3e"
              % (ks, ks, case, tile, k, e, ec, eh, eg[0], eg[1], eg[2], eg[3]))
        assert ec <= 1.5 * e + 5e-7, "step %d: c %.3e > %.3e" % (k, ec, 1.5 * e + 5e-7)
        assert eh <= 1.75 * e + 5e-7, "step %d: h %.3e > %.3e" % (k, eh, 1.75 * e + 5e-7)
        for q, slope in enumerate((0.25, 0.25, 0.25, 1.0)):
            assert eg[q] <= slope * e + 5e-7, "step %d: saved gate %d: %.3e > %.3e" % (k, q, eg[q], slope * e + 5e-7)


_LSTM_IDS = ["%s_h%d_%dx%d" % ("+".join(map(str, c[1])), c[2], c[3], c[4]) for c in T.LSTM_CASES]


@pytest.mark.parametrize("tile", T.DIRECT_TILES)
@pytest.mark.parametrize("case", T.LSTM_CASES, ids=_LSTM_IDS)
def test_convlstm_training_call_direct(case, tile):
    _lstm(case, 3, tile, M_TRAIN)


@pytest.mark.parametrize("tile", T.IGEMM_TILES)
@pytest.mark.parametrize("case", T.LSTM_CASES, ids=_LSTM_IDS)
def test_convlstm_training_call_igemm_1x1(case, tile):
    """kernel size 1: the implicit-GEMM route of rsis_convlstm_fwd (EPI_LSTM of conv_igemm.hip), held to M_IGEMM"""
    _lstm(case, 1, tile, M_IGEMM)
