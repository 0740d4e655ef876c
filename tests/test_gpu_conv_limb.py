"""The limb flavour of the direct 3x3 / stride 1 / pad 1 conv (rsis_amd/csrc/conv3x3_limb.h, RSIS_DTYPE_F32_LIMB: fp32 operands as three
bf16 limbs each, six products per K16 step on v_mfma_f32_32x32x16_bf16) against FLOAT64, through the C ABI into guarded buffers.
Cases: conv_limb_cases.py; data and float64 references: train_paths_cases.py / helpers.py, imported.

  * the packed copy: what rsis_conv_pack_fwd / _dgrad and the batched repack write is conv_limb_cases.limb_planes(), byte for byte;
  * EXACT regime: integers in -3..3 are single-limb values, so five of the six products are exact zeros, the sixth is the exact product and
    the fp32 accumulation is exact in any order (9 K + 6 < 2^24, asserted): outputs must EQUAL float64, default and deterministic mode;
  * ConvLSTM training call (act_out passed): c, h, the four saved gates at the bars of test_gpu_train_paths.py with M_LIMB, and the side
    max-pool keys against the h the call wrote;
  * one grouped call of three jobs of different sizes, two on the limb body (one per tile) and one on the f32 body: every job equals its
    single launch bit for bit;
  * NORMAL regime: err_gpu / err_host(chain model of the f32 kernel) printed per case and tile, held to M_LIMB = 2 x the worst measured."""
import numpy as np
import pytest
import torch

import conv_limb_cases as C
import train_paths_cases as T
from helpers import Guarded, assert_close, cell64, host_sums_conv, host_sums_dgrad, max_err as _err, to_tensor as _t

pytestmark = pytest.mark.gpu


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
    key = (kind, T.case_id(c), regime)
    if key not in _DATA:
        _DATA[key] = (T.fwd_data if kind == "fwd" else T.dgrad_data)(c, regime, T.case_seed(c))
    return _DATA[key]


def _params(cases):
    return [pytest.param(c, t, id="%s-t%d" % (T.case_id(c), t)) for c in cases for t in C.LIMB_TILES]


# ---------------------------------------------------------------- the packed copy
def _u16(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("case", C.PACK_CASES, ids=[c[0] for c in C.PACK_CASES])
def test_pack_writes_the_limb_planes(case):
    from rsis_amd import ops
    _name, cout, segs, offs, hid = case
    w = C.pack_weight(case)
    wd = _dev(w)
    pack = ops.PackedConv(3, segs, lstm_hid=hid, stride=1, pad=1, offs=offs, dtype=ops.DTYPE_F32_LIMB)
    want = {0: C.limb_planes(w, segs, offs, hid, False).reshape(-1), 1: C.limb_planes(w, segs, offs, hid, True).reshape(-1)}
    wp, wg = pack.fwd(wd), pack.dgrad(wd)
    torch.cuda.synchronize()
    assert wp.numel() * 2 == want[0].size and wg.numel() * 2 == want[1].size
    np.testing.assert_array_equal(_u16(wp), want[0])
    np.testing.assert_array_equal(_u16(wg), want[1])
    # ... and the batched repack that runs after the optimizer step rebuilds the same bytes
    wp.fill_(float("nan"))
    wg.fill_(float("nan"))
    ops.repack_all()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u16(wp), want[0])
    np.testing.assert_array_equal(_u16(wg), want[1])


def test_repack_after_a_copy_at_the_same_addresses():
    """the job table of the batched repack follows the copy, not its addresses: a second PackedConv with another geometry whose weight and
    copy sit exactly where those of an earlier one sat (what the allocator hands out after the first is freed) is packed by ITS job"""
    from rsis_amd import ops
    (_n1, cout1, segs1, offs1, hid1), (_n2, cout2, segs2, offs2, hid2) = C.PACK_CASES[0], C.PACK_CASES[1]
    w1, w2 = C.pack_weight(C.PACK_CASES[0]), C.pack_weight(C.PACK_CASES[1])
    buf = torch.zeros(max(w1.size, w2.size), device="cuda")
    a = ops.PackedConv(3, segs1, lstm_hid=hid1, stride=1, pad=1, offs=offs1, dtype=ops.DTYPE_F32_LIMB)
    wa = buf[:w1.size].view(w1.shape)
    wa.copy_(_t(w1))
    copy = a.fwd(wa)
    ops.repack_all()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u16(copy), C.limb_planes(w1, segs1, offs1, hid1, False).reshape(-1))
    del a
    b = ops.PackedConv(3, segs2, lstm_hid=hid2, stride=1, pad=1, offs=offs2, dtype=ops.DTYPE_F32_LIMB)
    wb = buf[:w2.size].view(w2.shape)
    wb.copy_(_t(w2))
    want = C.limb_planes(w2, segs2, offs2, hid2, False).reshape(-1)
    assert want.size == copy.numel() * 2 and wb.data_ptr() == wa.data_ptr()
    b.wp = copy                                       # (fwd() keeps a buffer of the right size)
    assert b.fwd(wb).data_ptr() == copy.data_ptr()
    copy.fill_(float("nan"))
    ops.repack_all()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u16(copy), want)


# ---------------------------------------------------------------- the calls
def run_fwd(c, d, tile, dtype=C.F32_LIMB):
    from rsis_amd import ops
    from rsis_amd._lib import check, int_array, lib, ptr, ptr_array, stream
    B, H, W = c["B"], c["H"], c["W"]
    pack = ops.PackedConv(3, c["segs"], stride=1, pad=1, dtype=dtype)
    wd, bd, ad = _dev(d["w"]), _dev(d["b"]), _dev(d["add"])
    wp = pack.fwd(wd)
    xs = [_dev(x) for x in d["xs"]]
    out = Guarded((B, c["cout"], H, W))
    check(lib().rsis_conv2d_fwd(ptr_array(xs), int_array(c["segs"]), len(xs), B, H, W, ptr(wp), c["cout"], 3, 1, 1, ptr(bd), ptr(ad), ptr(out.t), H, W,
                                tile + 100, dtype, stream()), "rsis_conv2d_fwd")
    torch.cuda.synchronize()
    out.check("forward output")
    return out.t


def run_dgrad(c, d, tile, dtype=C.F32_LIMB):
    from rsis_amd import ops
    from rsis_amd._lib import check, int_array, lib, ptr, ptr_array, stream
    B, H, W = c["B"], c["H"], c["W"]
    pack = ops.PackedConv(3, c["segs"], stride=1, pad=1, dtype=dtype)
    wd = pack.dgrad(_dev(d["w"]))
    dy = _dev(d["dy"])
    gs = [Guarded((B, s, H, W)) for s in c["segs"]]
    check(lib().rsis_conv2d_dgrad(ptr(dy), B, c["cout"], H, W, ptr(wd), pack.cin, 3, 1, 1, ptr_array([g.t for g in gs]), int_array(c["segs"]), len(gs),
                                  H, W, ptr(_dev(d["add"])), tile, dtype, stream()), "rsis_conv2d_dgrad")
    torch.cuda.synchronize()
    for i, g in enumerate(gs):
        g.check("dx[%d]" % i)
    return [g.t for g in gs]


# ---------------------------------------------------------------- 1. exact regime
@pytest.mark.parametrize("c,tile", _params(C.EXACT))
def test_limb_fwd_exact(c, tile, mode):
    assert T.exact_bound(c) < T.EXACT_LIMIT and all(s % 8 == 0 for s in c["segs"])
    d = _data("fwd", c, "exact")
    assert_close("forward, tile %d, exact" % tile, run_fwd(c, d, tile), d["ref"], 0.0)


@pytest.mark.parametrize("c,tile", _params(C.EXACT_DGRAD))
def test_limb_dgrad_exact(c, tile, mode):
    assert T.exact_bound(c, dgrad=True) < T.EXACT_LIMIT and c["cout"] % 8 == 0
    d = _data("dgrad", c, "exact")
    for i, (dx, ref) in enumerate(zip(run_dgrad(c, d, tile), d["refs"])):
        assert_close("dx[%d], tile %d, exact" % (i, tile), dx, ref, 0.0)


def test_inference_call_on_a_limb_copy_is_refused():
    """tile < 100 (no training marker) and a ConvLSTM call without act_out belong on the f32 copy: nothing is launched"""
    from rsis_amd import ops
    from rsis_amd._lib import int_array, lib, ptr, ptr_array, stream
    c = C.EXACT[3]
    d = _data("fwd", c, "exact")
    pack = ops.PackedConv(3, c["segs"], stride=1, pad=1, dtype=ops.DTYPE_F32_LIMB)
    wp = pack.fwd(_dev(d["w"]))
    xs = [_dev(x) for x in d["xs"]]
    out = Guarded((c["B"], c["cout"], c["H"], c["W"]))
    rc = lib().rsis_conv2d_fwd(ptr_array(xs), int_array(c["segs"]), 1, c["B"], c["H"], c["W"], ptr(wp), c["cout"], 3, 1, 1, None, None, ptr(out.t),
                               c["H"], c["W"], 0, ops.DTYPE_F32_LIMB, stream())
    torch.cuda.synchronize()
    assert rc == 3
    out.check("refused call")


# ---------------------------------------------------------------- 2. normal regime
_MODEL = {}


def _host_model(kind, c):
    key = (kind, T.case_id(c))
    if key not in _MODEL:
        d = _data(kind, c, "normal")
        if kind == "fwd":
            chain, _seg = host_sums_conv(d["xs"], d["w"], d["b"], 1, 1)
            ref = d["ref"]
        else:
            chain, _seg = host_sums_dgrad(d["dy"], d["w"], 1, 1, c["H"], c["W"])
            ref = torch.cat(d["refs"], 1)
        _MODEL[key] = _err(chain, ref)
    return _MODEL[key]


def _normal(kind, c, tile):
    from rsis_amd import ops
    d = _data(kind, c, "normal")
    K = (sum(c["segs"]) if kind == "fwd" else c["cout"]) * 9
    e_host = _host_model(kind, c)

    def call():
        if kind == "fwd":
            return run_fwd(c, d, tile).clone(), d["ref"]
        return torch.cat(run_dgrad(c, d, tile), 1), torch.cat(d["refs"], 1)

    prev = ops.set_deterministic(False)
    try:
        out, ref = call()
        e_gpu = _err(out, ref)
        print("\nLIMB %-6s %-34s tile %d: err gpu %.3e  host chain %.3e  ratio %.3f" % (kind, T.case_id(c), tile, e_gpu, e_host, e_gpu / e_host))
        assert C.M_LIMB <= 4.0
        assert_close("outer bar", out, ref, 2e-6 * np.sqrt(K) + 1e-6, 2e-6)
        assert e_gpu <= C.M_LIMB * e_host + 2e-7, "tight bar: %.3e > %.2f * %.3e + 2e-7" % (e_gpu, C.M_LIMB, e_host)
        ops.set_deterministic(True)
        det1, _ = call()
        det2, _ = call()
        assert torch.equal(det1, det2), "deterministic mode: two runs differ"
        assert torch.equal(det1, out), "the limb route is never split: both modes give the same bits"
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("c,tile", _params(C.NORMAL))
def test_limb_fwd_normal(c, tile):
    _normal("fwd", c, tile)


@pytest.mark.parametrize("c,tile", _params([dict(c, bias=False) for c in C.NORMAL]))
def test_limb_dgrad_normal(c, tile):
    _normal("dgrad", c, tile)


# ---------------------------------------------------------------- 3. ConvLSTM training call
_LSTM = {}


def _lstm_ref(case):
    key = (case[0], tuple(case[1])) + tuple(case[2:])
    if key not in _LSTM:
        B, segs, hid, H, W = case
        ctot = sum(segs) + hid
        seed = 9500 + 31 * (sum(segs) + 7 * hid + 3 * H + W)
        w, b = T.normal(seed, (4 * hid, ctot, 3, 3), 1.0 / np.sqrt(9 * ctot)), T.normal(seed + 1, (4 * hid,), 0.2)
        rs = np.random.default_rng(seed + 2)
        state = (_t(rs.uniform(-1, 1, (B, hid, H, W)).astype(np.float32)), _t(rs.uniform(-1, 1, (B, hid, H, W)).astype(np.float32)))
        steps = []
        for k, st in enumerate((None, state)):
            xs = [T.normal(seed + 10 * (k + 1) + i, (B, c, H, W)) for i, c in enumerate(segs)]
            h64, c64, g64 = cell64(w, b, xs, st)
            srcs = xs + ([st[0].numpy()] if st is not None else [])
            cin = sum(s.shape[1] for s in srcs)
            chain, _seg = host_sums_conv(srcs, np.ascontiguousarray(w[:, :cin]), b, 1, 1)
            i, f, o, g = g64.chunk(4, 1)
            act64 = torch.stack([torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)], 2)
            steps.append(dict(xs=xs, state=st, h64=h64, c64=c64, act64=act64, e_chain=_err(chain, g64)))
        _LSTM[key] = dict(w=w, b=b, steps=steps)
    return _LSTM[key]


class _LstmCall(object):
    """the device side of one ConvLSTM training call: sources, packed copy and guarded outputs (kept alive by the object)"""

    def __init__(self, case, k, limb, tile):
        from rsis_amd import ops
        B, segs, hid, H, W = case
        r = _lstm_ref(case)
        s = r["steps"][k]
        self.case, self.tile, self.step = case, tile, s
        self.dtype = ops.DTYPE_F32_LIMB if limb else ops.DTYPE_F32
        self.pack = ops.PackedConv(3, segs + [hid], lstm_hid=hid, stride=1, pad=1, dtype=self.dtype)
        self.keep = (_dev(r["w"]), _dev(r["b"]))
        self.wp = self.pack.fwd(*self.keep)
        self.srcs = [_dev(x) for x in s["xs"]] + ([s["state"][0].cuda()] if s["state"] is not None else [])
        self.cp = s["state"][1].cuda() if s["state"] is not None else None
        self.h, self.c, self.act = Guarded((B, hid, H, W)), Guarded((B, hid, H, W)), Guarded((B, 4 * hid, H, W))
        self.key = torch.zeros((B, hid), dtype=torch.int64, device="cuda")

    def fill(self, j):
        B, _segs, hid, H, W = self.case
        (j.B, j.H, j.W, j.Wp, j.bias_packed, j.addend, j.c_prev, j.h_out, j.c_out, j.act_out, j.hid, j.ks, j.pad, j.tile, j.dtype, j.side_key) = (
            B, H, W, self.wp.data_ptr(), self.pack.bias_p.data_ptr(), None, self.cp.data_ptr() if self.cp is not None else None, self.h.t.data_ptr(),
            self.c.t.data_ptr(), self.act.t.data_ptr(), hid, 3, 1, self.tile, self.dtype, self.key.data_ptr())
        j.nsrc = len(self.srcs)
        for i, s in enumerate(self.srcs):
            j.src[i], j.Csrc[i] = s.data_ptr(), s.shape[1]

    def check_guards(self):
        for g, what in ((self.h, "h"), (self.c, "c"), (self.act, "act_out")):
            g.check(what)


def _run_lstm(calls):
    from rsis_amd import _lib
    from rsis_amd._lib import check, lib, stream
    jobs = (_lib.LstmJob * len(calls))()
    for j, q in zip(jobs, calls):
        q.fill(j)
    check(lib().rsis_convlstm_fwd_batch(jobs, len(calls), stream()), "rsis_convlstm_fwd_batch")
    torch.cuda.synchronize()
    for q in calls:
        q.check_guards()


def _key_decode(key):
    """(value, pixel index) of rsis_side_key keys (common.h): order-preserving bits << 32 | 0x7FFFFFFF - index"""
    k = key.cpu().numpy().astype(np.uint64)
    u = (k >> np.uint64(32)).astype(np.uint32)
    u = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)
    return u.view(np.float32), 0x7FFFFFFF - (k & np.uint64(0xFFFFFFFF)).astype(np.int64)


@pytest.mark.parametrize("tile", C.LIMB_TILES)
@pytest.mark.parametrize("k", [0, 1], ids=["zero_state", "uniform_state"])
@pytest.mark.parametrize("case", C.LSTM, ids=["h%d" % c[2] for c in C.LSTM])
def test_limb_convlstm_training_call(case, k, tile, mode):
    B, _segs, hid, H, W = case
    q = _LstmCall(case, k, True, tile)
    _run_lstm([q])
    s = q.step
    e = C.M_LIMB * s["e_chain"] + 2e-7
    ec, eh = _err(q.c.t, s["c64"]), _err(q.h.t, s["h64"])
    got = q.act.t.double().cpu().view(B, hid, 4, H, W)
    eg = [float((got[:, :, g] - s["act64"][:, :, g]).abs().max()) for g in range(4)]
    print("\nLIMB-LSTM %r tile %d step %d: e %.3e  err c %.3e  h %.3e  gates i %.3e f %.3e o %.3e g %.3e" % (case, tile, k, e, ec, eh, *eg))
    assert ec <= 1.5 * e + 5e-7 and eh <= 1.75 * e + 5e-7
    for g, slope in enumerate((0.25, 0.25, 0.25, 1.0)):
        assert eg[g] <= slope * e + 5e-7, "saved gate %d: %.3e > %.3e" % (g, eg[g], slope * e + 5e-7)
    # the side max-pool keys: the largest h of every (image, hidden channel) plane of the h the call wrote, at its first pixel
    val, idx = _key_decode(q.key)
    hf = q.h.t.cpu().numpy().reshape(B, hid, H * W)
    np.testing.assert_array_equal(val, hf.max(2))
    np.testing.assert_array_equal(idx, hf.argmax(2))


# ---------------------------------------------------------------- 4. the grouped call
def test_grouped_call_equals_the_single_launches():
    """three jobs of different sizes in ONE grid (default mode: the deterministic mode launches one by one): two on the limb body, one
    per tile, one on the f32 body; each must equal its single launch bit for bit"""
    from rsis_amd import ops
    prev = ops.set_deterministic(False)
    try:
        single = [_LstmCall(g["case"], 1, g["limb"], g["tile"]) for g in C.GROUP]
        for q in single:
            _run_lstm([q])
        grouped = [_LstmCall(g["case"], 1, g["limb"], g["tile"]) for g in C.GROUP]
        _run_lstm(grouped)
        for n, (a, b) in enumerate(zip(single, grouped)):
            for what in ("h", "c", "act"):
                assert torch.equal(getattr(a, what).t, getattr(b, what).t), "job %d: %s differs from the single launch" % (n, what)
            assert torch.equal(a.key, b.key), "job %d: side keys differ" % n
            assert _err(b.h.t, b.step["h64"]) < 1e-4
    finally:
        ops.set_deterministic(prev)


def test_grouped_gradients_equal_the_single_launches():
    """rsis_conv2d_dgrad_batch: a limb job per tile and an f32 job in one grid, two destinations each where the case has two sources"""
    from rsis_amd import _lib, ops
    from rsis_amd._lib import check, lib, stream
    prev = ops.set_deterministic(False)
    try:
        specs = [(dict(c, addend=False), limb, tile) for c, limb, tile in ((C.EXACT_DGRAD[1], True, 5), (C.EXACT_DGRAD[3], False, 4), (C.EXACT_DGRAD[2], True, 4))]
        singles = []
        for c, limb, tile in specs:
            singles.append(run_dgrad(c, _data("dgrad", c, "normal"), tile, ops.DTYPE_F32_LIMB if limb else ops.DTYPE_F32))
        jobs = (_lib.DgradJob * len(specs))()
        keep, outs = [], []
        for j, (c, limb, tile) in zip(jobs, specs):
            d = _data("dgrad", c, "normal")
            dt = ops.DTYPE_F32_LIMB if limb else ops.DTYPE_F32
            pack = ops.PackedConv(3, c["segs"], stride=1, pad=1, dtype=dt)
            w = _dev(d["w"])
            wd, dy = pack.dgrad(w), _dev(d["dy"])
            gs = [Guarded((c["B"], s, c["H"], c["W"])) for s in c["segs"]]
            keep.append((pack, w, wd, dy))
            outs.append(gs)
            (j.dy, j.B, j.Cout, j.Hy, j.Wy, j.Wd, j.Cin_packed, j.ks, j.stride, j.pad, j.ndst, j.Hx, j.Wx, j.addend, j.tile, j.dtype) = (
                dy.data_ptr(), c["B"], c["cout"], c["H"], c["W"], wd.data_ptr(), pack.cin, 3, 1, 1, len(gs), c["H"], c["W"], None, tile, dt)
            for i, g in enumerate(gs):
                j.dx[i], j.Cdx[i] = g.t.data_ptr(), c["segs"][i]
        check(lib().rsis_conv2d_dgrad_batch(jobs, len(specs), stream()), "rsis_conv2d_dgrad_batch")
        torch.cuda.synchronize()
        for n, (gs, ss) in enumerate(zip(outs, singles)):
            for i, (g, s) in enumerate(zip(gs, ss)):
                g.check("job %d dx[%d]" % (n, i))
                assert torch.equal(g.t, s), "job %d dx[%d] differs from the single launch" % (n, i)
    finally:
        ops.set_deterministic(prev)
