"""Case tables, input builders, float64 references, rounding helpers and host models of test_gpu_blk_paths.py (and of
test_blk_paths_host.py, which checks them without a device): the channel-blocked bf16 convs of csrc/conv_blk.hip, the BatchNorm and
the layout helpers of csrc/blk_norm.hip.  Everything here is numpy / torch on the host; nothing imports the library.

  blk tensor        : logical [B][C][H][W] stored as bf16 [B][C/8][H][W][8];
  float64 reference : the operation on the SAME bf16-valued inputs, every intermediate in float64;
  exact regime      : inputs for which every fp32 operation of the kernel is exact in any order (small integers), so the stored value
                      must EQUAL bf16_rne64(reference): the ONE round-to-nearest-even the kernels promise;
  normal regime     : nearest_check -- the stored value is the bf16 nearest to the reference, or, where the reference lies within
                      `delta` (a derived bound of the kernel's fp32 error) of a midpoint between two bf16 values, one of the two."""
import numpy as np

U24 = 2.0 ** -24                      # one fp32 rounding, relative
F32 = np.float32
GUARD_BLK = 128                       # sentinel elements on each side of a GuardedBlk view (256 bytes: the view stays 16-byte aligned)

_MASK45 = np.uint64((1 << 45) - 1)    # float64 mantissa bits below the 7 that bf16 keeps
_BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
_BF16_MIN_NORMAL = 2.0 ** -126
_BF16_DENORM = 2.0 ** -133            # spacing of the bf16 denormals


def _rng(seed):
    return np.random.default_rng(seed)


# ======================================================================================================================
# 1. bf16 rounding on float64
# ======================================================================================================================
def bf16_rne64(a):
    """the bf16 value nearest to each float64, ties to even, as float64 -- on the float64 bit pattern (no float32 on the way, so no
    double rounding): keep 7 of the 52 mantissa bits; below 2^-126 the grid is the denormals' 2^-133.  NaN stays NaN, +-inf and +-0 stay."""
    a = np.array(a, np.float64, copy=True)
    out = a.copy()
    fin = np.isfinite(a)
    mag = np.abs(a)
    nrm = fin & (mag >= _BF16_MIN_NORMAL)
    bits = mag[nrm].view(np.uint64)
    lsb = (bits >> np.uint64(45)) & np.uint64(1)
    bits = (bits + np.uint64((1 << 44) - 1) + lsb) & ~_MASK45
    r = bits.view(np.float64)
    r = np.where(r > _BF16_MAX, np.inf, r)
    out[nrm] = np.copysign(r, a[nrm])
    den = fin & ~nrm
    out[den] = np.copysign(np.rint(mag[den] / _BF16_DENORM) * _BF16_DENORM, a[den])      # np.rint: half to even; both scalings exact
    return out


def bf16_floor_ulp(mag):
    """(largest bf16 value <= mag, distance to the next bf16 value above it) for finite mag >= 0"""
    mag = np.array(mag, np.float64, copy=True)
    lo = mag.copy()
    nrm = mag >= _BF16_MIN_NORMAL
    lo[nrm] = (mag[nrm].view(np.uint64) & ~_MASK45).view(np.float64)
    lo[~nrm] = np.floor(mag[~nrm] / _BF16_DENORM) * _BF16_DENORM
    _m, e = np.frexp(np.maximum(lo, _BF16_MIN_NORMAL))          # lo in [2^(e-1), 2^e)
    ulp = np.ldexp(1.0, e - 8)
    return lo, ulp


def bf16_neighbours(a):
    """the two adjacent bf16 values lo <= |a| < hi with the sign of a (a itself = lo when it is a bf16 value)"""
    a = np.asarray(a, np.float64)
    lo, ulp = bf16_floor_ulp(np.abs(a))
    return np.copysign(lo, a), np.copysign(lo + ulp, a)


def mid_dist(a):
    """distance of |a| to the nearest midpoint between two adjacent bf16 values (the midpoint of its own interval, of the one below or
    of the one above: next to a binade boundary the interval below is half as wide)"""
    mag = np.abs(np.asarray(a, np.float64))
    lo, ulp = bf16_floor_ulp(mag)
    d = np.abs(mag - (lo + 0.5 * ulp))
    _l2, ulp_up = bf16_floor_ulp(lo + ulp)
    d = np.minimum(d, np.abs(lo + ulp + 0.5 * ulp_up - mag))
    below = lo > 0
    l3, ulp_dn = bf16_floor_ulp(np.where(below, lo - 0.25 * ulp, 0.0))      # a value inside the interval below
    d = np.where(below, np.minimum(d, np.abs(mag - (l3 + 0.5 * ulp_dn))), d)
    return d


def is_bf16(a):
    a = np.asarray(a, np.float64)
    return bf16_rne64(a) == a


def is_tie(a):
    return mid_dist(a) == 0.0


def trunc_bf16(a):
    """defect model: the store truncates (round toward zero)"""
    return bf16_neighbours(a)[0]


def half_away_bf16(a):
    """defect model: round to nearest, ties AWAY from zero"""
    lo, hi = bf16_neighbours(a)
    mag = np.abs(np.asarray(a, np.float64))
    return np.where(mag - np.abs(lo) >= np.abs(hi) - mag, hi, lo)


def undecided(ref, delta):
    """elements of a normal case that nearest_check cannot pin to one value: within delta of a midpoint, and not an exact zero"""
    ref = np.asarray(ref, np.float64)
    return (mid_dist(ref) <= delta) & (ref != 0)


UNDECIDED_CAP = 0.01                  # a condition on the INPUTS of a normal case: at most 1 % of its elements may be undecided


def nearest_check(got_bf16, ref64, delta):
    """ok[...] per element: got == bf16_rne64(ref), or mid_dist(ref) <= delta and got is one of the two bf16 neighbours of ref.
    ref == 0 with got == 0 (an exact zero behind a ReLU) passes under the first rule, either sign of zero.
    Where delta exceeds HALF A bf16 STEP of the reference (a value that is nearly zero by cancellation of large terms) no two
    neighbours can be named: such an element is undecided by construction (mid_dist <= step / 2 <= delta: it counts toward the 1 % cap)
    and must lie within delta + step / 2 of the reference."""
    got = np.asarray(got_bf16, np.float64)
    ref = np.asarray(ref64, np.float64)
    delta = np.broadcast_to(np.asarray(delta, np.float64), ref.shape)
    assert got.shape == ref.shape
    ok = got == bf16_rne64(ref)
    lo, hi = bf16_neighbours(ref)
    und = undecided(ref, delta)
    step = np.abs(hi - lo)
    wide = (ref != 0) & (delta > step / 2) & (np.abs(got - ref) <= delta + step / 2)
    return ok | (und & ((got == lo) | (got == hi))) | wide


def assert_nearest(what, got_bf16, ref64, delta, where=None):
    got, ref = np.asarray(got_bf16, np.float64), np.asarray(ref64, np.float64)
    ok = nearest_check(got, ref, delta)
    if where is not None:
        ok = ok | ~where
    if not ok.all():
        i = np.unravel_index(int(np.argmin(ok)), ok.shape)
        d = np.broadcast_to(np.asarray(delta, np.float64), ref.shape)
        raise AssertionError("%s: %d of %d elements are not the nearest bf16 of the float64 reference; first at %s: got %.9g, reference %.9g "
                             "(nearest %.9g), mid_dist %.3e, delta %.3e" % (what, int((~ok).sum()), ok.size, i, got[i], ref[i],
                                                                           float(bf16_rne64(ref[i])), float(mid_dist(ref[i])), d[i]))


class GuardedBlk(object):
    """a bf16 output as a view into one larger allocation: GUARD_BLK sentinel elements on each side, the view prefilled with a non-zero
    pattern (a kernel that skips an element leaves it).  .t is the view, .check() asserts that both zones still hold the sentinel.
    (The integer counterpart is GuardedInt of test_gpu_loss_path.py, the fp32 one helpers.Guarded.)"""
    SENTINEL = 0x7A5A                 # bf16 bits: 2.83e35
    PREFILL = 0x4049                  # bf16 bits: 3.140625

    def __init__(self, shape, device="cuda"):
        import torch
        n = int(np.prod(shape))
        self.n = n
        self.buf = torch.full((n + 2 * GUARD_BLK,), self.SENTINEL, dtype=torch.int16, device=device)
        self.buf[GUARD_BLK:GUARD_BLK + n] = self.PREFILL
        self.t = self.buf[GUARD_BLK:GUARD_BLK + n].view(torch.bfloat16).view(*shape)

    def check(self, what="output"):
        lo, hi = self.buf[:GUARD_BLK], self.buf[GUARD_BLK + self.n:]
        assert hi.numel() == GUARD_BLK
        assert bool((lo == self.SENTINEL).all()), "%s: the guard zone in FRONT of the tensor was written" % what
        assert bool((hi == self.SENTINEL).all()), "%s: the guard zone BEHIND the tensor was written" % what

    def untouched(self):
        return bool((self.t.view(-1).view(self.buf.dtype) == self.PREFILL).all())


def to_blk64(x):
    """[B][C][H][W] -> [B][C/8][H][W][8] (numpy, any dtype)"""
    B, C, H, W = x.shape
    return np.ascontiguousarray(x.reshape(B, C // 8, 8, H, W).transpose(0, 1, 3, 4, 2))


def from_blk64(y):
    B, Cb, H, W, _ = y.shape
    return np.ascontiguousarray(y.transpose(0, 1, 4, 2, 3).reshape(B, Cb * 8, H, W))


# ======================================================================================================================
# 2. rsis_blk_conv2d / rsis_blk_conv2d_bn_eval, exact regime
# ======================================================================================================================
def _cv(B, Cin, Cout, H, W, ks, role, why):
    return dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, ks=ks, role=role, why=why)


# role "index": every output is itself a bf16 value (|y| small): one missing or doubled tap of +-1 shows.
# role "round": many outputs are NOT bf16 values and many are exact ties: the rounding mode of the store shows.
# role "tie"  : counts toward the tie condition only.
# 3x3: ring stage = 16 input channels (nq = ceil(Cin / 16)), NR = 3.  1x1: stage = 32 channels (nq = ceil(Cin / 32)), NR = 4, the map
# flattened to H * W pixels per image and cut into 64- / 128-pixel tiles.
CONV_CASES = [
    _cv(2, 8, 8, 5, 5, 3, "index", "nq 1 with a ragged stage (8 of 16 channels); 5 x 5 map; Cout 8; 2 pixel tiles of 8 x 8 (not a multiple of 8)"),
    _cv(2, 24, 24, 9, 11, 3, "index", "nq 2, ragged last stage; 9 x 11; Cout 24; W <= 16 branch"),
    _cv(1, 40, 40, 10, 13, 3, "index", "nq 3 = NR, ragged last stage; 10 x 13; Cout 40: just above a 32-row block"),
    _cv(2, 64, 64, 9, 17, 3, "index", "nq 4 > NR; W = 17 > 16: the widest dispatch branch, a second ragged tile column; Cout 64 = one block's rows"),
    _cv(1, 48, 136, 1, 1, 3, "index", "nq 3 full stages; a 1 x 1 map (centre tap only); Cout 136: just above 128 rows"),
    _cv(1, 256, 64, 14, 14, 3, "round", "layer-3 3x3: deep ring"),
    _cv(3, 512, 24, 7, 7, 3, "round", "layer-4 3x3, B = 3: nq 32; W <= 8 branch"),
    _cv(1, 8, 8, 1, 1, 1, "index", "nq 1 ragged (8 of 32 channels); a single pixel"),
    _cv(3, 40, 24, 9, 11, 1, "index", "nq 2, ragged last stage; 99 pixels per image, B = 3: tiles end inside the allocation of the next image"),
    _cv(2, 72, 136, 17, 9, 1, "index", "nq 3: the first count that fills the 1x1 prologue (NR - 1 = 3 chunks in flight); 153 pixels: two 128-pixel tiles; Cout 136"),
    _cv(2, 128, 40, 5, 5, 1, "index", "nq 4 full stages; H W = 25 <= 64 branch; Cout 40"),
    _cv(2, 136, 64, 10, 13, 1, "index", "nq 5, ragged last stage; 130 pixels: one over a 128-pixel tile"),
    _cv(1, 2048, 32, 7, 7, 1, "round", "layer-4 1x1: nq 64"),
    _cv(1, 1024, 64, 9, 11, 1, "tie", "nq 32 on a ragged map"),
]
CONV_VARIANTS = {3: (0, 1, 2, 3, 4, 5, 6), 1: (0, 1, 2, 3, 4, 5)}
MIN_NOT_BF16, MIN_TIES = 0.05, 0.02   # rounding cases: share of outputs that are not bf16 values / that are exact ties


def conv_id(c):
    return "b%d_%dto%d_%dx%d_k%d" % (c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["ks"])


def conv_seed(c):
    return (c["B"] * 7 + c["Cin"] * 131 + c["Cout"] * 17 + c["H"] * 1009 + c["W"] * 53 + c["ks"]) % 100003


def _ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def conv64(x, w, transpose=False):
    """stride-1 'same' conv (or conv_transpose: the data gradient) in float64"""
    import torch
    import torch.nn.functional as Fn
    f = Fn.conv_transpose2d if transpose else Fn.conv2d
    return f(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(w)), padding=w.shape[-1] // 2).numpy()


def conv_exact_data(c):
    """integers in -3..3 for x, dy, w and the addend (all exact in bf16): forward y = conv(x, w), data gradient dx = conv^T(dy, w) + addend.
    abs_* = sum |terms| per output (the fp32 accumulation is exact in any order, MFMA included, while it stays below 2^24)."""
    rng = _rng(conv_seed(c))
    B, Cin, Cout, H, W, ks = (c[k] for k in ("B", "Cin", "Cout", "H", "W", "ks"))
    wmax = 1 if c["role"] == "index" and Cin * ks * ks > 100 else 3        # (index cases: |y| stays below 256, so every output is a bf16 value)
    x, w = _ints(rng, (B, Cin, H, W)), _ints(rng, (Cout, Cin, ks, ks), -wmax, wmax)
    dy, add = _ints(rng, (B, Cout, H, W)), _ints(rng, (B, Cin, H, W))
    y = conv64(x, w)
    dx = conv64(dy, w, transpose=True) + add
    return dict(x=x, w=w, dy=dy, add=add, y=y, dx=dx, abs_y=conv64(np.abs(x), np.abs(w)),
                abs_dx=conv64(np.abs(dy), np.abs(w), transpose=True) + np.abs(add))


# ---- eval-mode BatchNorm in the conv's epilogue: sc = gamma * rsqrt(var + 0), sh = beta - mean * sc, all exact powers of two ----
BN_EVAL_CASES = [CONV_CASES[5], CONV_CASES[12]]        # one rounding case per kernel family
BN_EVAL_MIN_DIFF = 0.01               # the two rounding modes must differ on at least 1 % of the elements
RSQRT_POW2 = (0.0625, 0.25, 1.0, 4.0, 16.0)     # arguments at which rsqrtf must be exact (probed on the device): 4, 2, 1, 1/2, 1/4


def bn_eval_params(c):
    """gamma, beta, mean, var per output channel (fp32-exact powers of two, eps = 0), the resulting sc / sh, and a +-integer residual"""
    rng = _rng(conv_seed(c) + 1)
    Cout = c["Cout"]
    var = np.array(RSQRT_POW2)[rng.integers(0, len(RSQRT_POW2), Cout)]
    gamma = 2.0 ** rng.integers(-2, 2, Cout) * rng.choice([-1.0, 1.0], Cout)
    half = np.arange(Cout) % 2 == 0
    beta = np.where(half, 2.0 ** rng.integers(-2, 3, Cout) * rng.choice([-1.0, 1.0], Cout), 0.0)
    mean = np.where(half, 0.0, 2.0 ** rng.integers(-2, 3, Cout) * rng.choice([-1.0, 1.0], Cout))
    sc = gamma / np.sqrt(var)
    sh = beta - mean * sc
    res = _ints(rng, (c["B"], Cout, c["H"], c["W"]))
    return dict(gamma=gamma, beta=beta, mean=mean, var=var, sc=sc, sh=sh, res=res)


def bn_eval_expect(y64, p, res, relu, single_rounding, store=bf16_rne64):
    """the two promised results: single_rounding = 0 -- the affine map of the bf16-ROUNDED product, rounded again; 1 -- of the exact product,
    rounded once.  (The affine map and the residual add are exact in fp32: integers below 2^11 times 2^k plus 2^j plus a small integer.)"""
    v = y64 if single_rounding else store(y64)
    o = v * p["sc"][None, :, None, None] + p["sh"][None, :, None, None]
    if res is not None:
        o = o + res
    if relu:
        o = np.maximum(o, 0.0)
    return store(o)


# ---- rsis_blk_conv3x3_batch, plain epilogue (csrc/conv_blk_dec.hip: bd_body tiles 4 = 32 rows x 16 x 8 px, 5 = 32 rows x 32 x 8 px) ----
def _bt(B, segs, Cout, H, W, split, role, why):
    return dict(B=B, segs=segs, Cin=sum(segs), Cout=Cout, H=H, W=W, ks=3, split=split, role=role, why=why)


BATCH_CASES = [
    _bt(2, [8], 8, 5, 5, None, "index", "one source with a ragged stage; Cout 8: one destination"),
    _bt(3, [24, 8, 40], 48, 10, 13, (24, 24), "index", "three sources, each with its own channel tail; destinations split at row 24: inside a 32-row block"),
    _bt(2, [16, 8], 40, 9, 17, (8, 32), "index", "two sources; W = 17: a second, ragged 16-pixel tile column; destinations 8 | 32"),
    _bt(1, [128, 128], 64, 14, 14, (32, 32), "round", "the rounding case of this kernel family: 256 input channels"),
]
BATCH_TILES = (0, 1, 4, 5)


def batch_id(c):
    return "b%d_%sto%d_%dx%d" % (c["B"], "+".join(str(v) for v in c["segs"]), c["Cout"], c["H"], c["W"])


def batch_exact_data(c):
    """conv_exact_data over the channel concat of the sources, plus an integer bias and an addend of the OUTPUT's shape:
    y = conv(cat(xs), w), yb = y + bias + add_out;  data gradient dx = conv^T(dy, w) (no addend), split back over the sources"""
    d = conv_exact_data(c)
    rng = _rng(conv_seed(c) + 2)
    bias, add_out = _ints(rng, (c["Cout"],)), _ints(rng, d["y"].shape)
    d.update(bias=bias, add_out=add_out, yb=d["y"] + bias[None, :, None, None] + add_out, dx0=d["dx"] - d["add"],
             abs_yb=d["abs_y"] + np.abs(bias)[None, :, None, None] + np.abs(add_out))
    return d


# ---- ConvLSTM epilogue of rsis_blk_conv3x3_batch: c = f c_prev + i g, h = o tanh(c) on the hardware's exp2 / rcp units ----
LOG2E = float(F32(1.4426950408889634))
E_F = 1.71e-7                         # worst absolute error of rsis_sigmoid_fast / rsis_tanh_fast against float64, probed on the device: 1.705e-7 (NOTES.md (93))
# With EXACT pre-activations (dyadic data) the only errors are those of the two functions (E_F each, their own rounding included) and
# a few fp32 roundings.  The issue's chain (sigmoid' <= 1/4, tanh' <= 1, |c_prev| <= 1, |gates| <= 1):
#   c = f c_prev + i g         -> 2.25 E_F + 4 u max(1, |c|)
#   act (i, f, o, g)           -> E_F
#   h = o tanh(c)              -> E_F |tanh c| + |o| (E_F + dc) <= 2 E_F + dc


def lstm_delta_c(c64):
    return 2.25 * E_F + 4.0 * U24 * np.maximum(1.0, np.abs(c64))


def lstm_delta_h(c64):
    return 2.0 * E_F + lstm_delta_c(c64)


def sigmoid_fast32(x):
    """rsis_sigmoid_fast (common.h) in numpy float32: rcp(1 + exp2(-log2(e) x)), each operation rounded to fp32"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp2(F32(-LOG2E) * x).astype(F32))).astype(F32)


def tanh_fast32(x):
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        return (F32(2) * (F32(1) / (F32(1) + np.exp2(F32(-2.0 * LOG2E) * x).astype(F32))).astype(F32) - F32(1)).astype(F32)


def fast_probe_args():
    """the arguments of the device probe: EVERY gate pre-activation of the ConvLSTM and side-key cases (lstm_pre_values: the bars rest on
    what is measured), within every multiple of 1 / 32 in [-8, 8] and of 1 / 4 up to +-24.  All are bf16 values: the probe passes them
    through the blk addend."""
    v = np.unique(np.concatenate([np.arange(-256, 257) / 32.0, np.arange(-96, 97) / 4.0, lstm_pre_values()]))
    assert is_bf16(v).all(), "a pre-activation of the cases cannot be passed through the bf16 addend of the probe"
    return v


def _lc(B, hid, c_up, H, W, why):
    return dict(B=B, hid=hid, c_up=c_up, H=H, W=W, why=why)


LSTM_CASES = [
    _lc(2, 8, 8, 10, 13, "hid 8: one 32-row block; an 8-channel source besides the state"),
    _lc(1, 16, 0, 9, 17, "hid 16; no source besides the state: zero state runs nsrc = 0 (gates = addend); W = 17: a ragged second tile column"),
    _lc(2, 24, 16, 5, 5, "hid 24: 4 hid = 96 rows, a partial 128-row group"),
]
LSTM_TILES = (4, 5)


def lstm_id(c):
    return "b%d_hid%d_up%d_%dx%d" % (c["B"], c["hid"], c["c_up"], c["H"], c["W"])


def lstm_data(c, state):
    """dyadic cell inputs: the source `up` integers in -2..2, h_prev multiples of 1 / 8 in [-1, 1], c_prev in [-1/2, 1/2], weights [4 hid][c_up + hid]
    in {0, +-1/4} with 1 in 8 non-zero, the addend G (reference rows [i | f | o | g] x hid) multiples of 1 / 4 in [-2, 2]: every gate
    pre-activation is a multiple of 1 / 32 with sum |terms| far below 2^24 / 32, exact in fp32 in any order.  state False: zero state
    (c_prev = NULL, no h_prev source)."""
    rng = _rng(c["hid"] * 1009 + c["H"] * 53 + c["W"] + int(state))
    B, hid, cu, H, W = c["B"], c["hid"], c["c_up"], c["H"], c["W"]
    up = _ints(rng, (B, cu, H, W), -2, 2) if cu else None
    h_prev, c_prev = _ints(rng, (B, hid, H, W), -8, 8) / 8.0, _ints(rng, (B, hid, H, W), -4, 4) / 8.0
    w = _ints(rng, (4 * hid, cu + hid, 3, 3), -1, 1) * (rng.random((4 * hid, cu + hid, 3, 3)) < 0.125) / 4.0
    # (the i and o pre-activations lean positive and the g pre-activation stays away from 0, so that few |h| are tiny: an h below 0.01 has
    #  a bf16 step under 1e-4 against a delta of 1e-6, and the share of undecided elements is a condition on these inputs)
    G = _ints(rng, (B, 4 * hid, H, W), -8, 8) / 4.0
    G[:, :hid] = _ints(rng, (B, hid, H, W), -2, 8) / 4.0
    G[:, 2 * hid:3 * hid] = _ints(rng, (B, hid, H, W), -2, 8) / 4.0
    G[:, 3 * hid:] = _ints(rng, (B, hid, H, W), 4, 8) / 4.0 * np.where(rng.random((B, hid, H, W)) < 0.5, -1.0, 1.0)
    parts = ([up] if cu else []) + ([h_prev] if state else [])
    cols = list(range(cu)) + (list(range(cu, cu + hid)) if state else [])
    if parts:
        xin = np.concatenate(parts, 1)
        pre, abs_pre = G + conv64(xin, w[:, cols]), np.abs(G) + conv64(np.abs(xin), np.abs(w[:, cols]))
    else:
        pre, abs_pre = G.copy(), np.abs(G)
    ai, af, ao, ag = np.split(pre, 4, 1)
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    gi, gf, go, gg = sig(ai), sig(af), sig(ao), np.tanh(ag)
    c64 = gf * (c_prev if state else 0.0) + gi * gg
    return dict(up=up, h_prev=h_prev if state else None, c_prev=c_prev if state else None, w=w, G=G, pre=pre, abs_pre=abs_pre,
                act=np.concatenate([gi, gf, go, gg], 1), c=c64, h=go * np.tanh(c64))


def lstm_model32(d):
    """the epilogue in numpy float32 on the exact pre-activations: (c, h, act) with h / act unrounded fp32 values as float64"""
    ai, af, ao, ag = np.split(d["pre"].astype(F32), 4, 1)
    gi, gf, go, gg = sigmoid_fast32(ai), sigmoid_fast32(af), sigmoid_fast32(ao), tanh_fast32(ag)
    cp = d["c_prev"].astype(F32) if d["c_prev"] is not None else F32(0)
    c = (gf.astype(np.float64) * cp + (gi * gg).astype(F32)).astype(F32)
    h = (go * tanh_fast32(c)).astype(F32)
    return c.astype(np.float64), h.astype(np.float64), np.concatenate([gi, gf, go, gg], 1).astype(np.float64)


# ---- side keys of the ConvLSTM epilogue (global max-pool of h: value and the SMALLEST pixel index attaining it) ----
SIDE_CHECK_TILES = 192                # RSIS_SIDE_CHECK_TILES (common.h): from that many tiles per image on, a block reads the key before its atomic


def _sk(B, hid, csrc, H, W, tile, why):
    return dict(B=B, hid=hid, csrc=csrc, H=H, W=W, tile=tile, why=why)


SIDE_CASES = [
    _sk(2, 24, 0, 10, 13, 5, "no source (gates = addend), hid 24: 4 hid = 96 rows, a partial 128-row group; tile 5"),
    _sk(1, 8, 8, 96, 256, 4, "12 x 16 = 192 tiles of 16 x 8: RSIS_SIDE_CHECK_TILES exactly, the path that reads the key first"),
    _sk(1, 8, 8, 88, 256, 4, "11 x 16 = 176 tiles: the path without the check"),
]


def side_id(c):
    return "b%d_hid%d_src%d_%dx%d_t%d" % (c["B"], c["hid"], c["csrc"], c["H"], c["W"], c["tile"])


def side_tiles(c):
    tw = 32 if c["tile"] == 5 else 16
    return -(-c["W"] // tw) * -(-c["H"] // 8)


def side_data(c, tie):
    """dyadic inputs of a ConvLSTM cell with zero state: x integers in -2..2, weights in {0, +-1/4} with 1 in 8 non-zero (tie: all zero),
    addend G (reference row order [i | f | o | g] x hid) multiples of 1/4 in -2..2 shaped as in lstm_data (i and o lean positive, g stays
    away from 0: few tiny |h|), constant over the pixels when `tie`; every pre-activation is then a multiple of 1/16 below 2^8: exact
    in fp32.  Returns the float64 c, h and act (reference row order) as well."""
    rng = _rng(c["H"] * 1009 + c["W"] * 53 + c["hid"] + int(tie))
    B, hid, cs, H, W = c["B"], c["hid"], c["csrc"], c["H"], c["W"]
    x = _ints(rng, (B, cs, H, W), -2, 2) if cs else None
    w = np.zeros((4 * hid, max(cs, 8), 3, 3))
    if not tie and cs:
        w = _ints(rng, w.shape, -1, 1) * (rng.random(w.shape) < 0.125) / 4.0
    gs = (B, hid, 1, 1) if tie else (B, hid, H, W)
    G = np.concatenate([_ints(rng, gs, -2, 8), _ints(rng, gs, -8, 8), _ints(rng, gs, -2, 8),
                        _ints(rng, gs, 4, 8) * np.where(rng.random(gs) < 0.5, -1.0, 1.0)], 1) / 4.0
    G = np.broadcast_to(G, (B, 4 * hid, H, W)).copy()
    pre = G + (conv64(x, w[:, :cs]) if cs else 0.0)
    ai, af, ao, ag = np.split(pre, 4, 1)
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    gi, gf, go, gg = sig(ai), sig(af), sig(ao), np.tanh(ag)
    c64 = gi * gg
    return dict(x=x, w=w, G=G, pre=pre, c=c64, h=go * np.tanh(c64), act=np.concatenate([gi, gf, go, gg], 1))


_PRE_VALUES = []


def lstm_pre_values():
    """every gate pre-activation that occurs in LSTM_CASES (both states) and SIDE_CASES (tie and spread)"""
    if _PRE_VALUES:
        return _PRE_VALUES[0]
    v = [lstm_data(c, st)["pre"].reshape(-1) for c in LSTM_CASES for st in (False, True)]
    v += [side_data(c, tie)["pre"].reshape(-1) for c in SIDE_CASES for tie in (True, False)]
    _PRE_VALUES.append(np.unique(np.concatenate(v)))
    return _PRE_VALUES[0]


def key_decode(key):
    """(value, flat pixel) of the 64-bit side keys (numpy int64): the order-preserving image of the fp32 value above 0x7FFFFFFF - pixel"""
    key = np.asarray(key).astype(np.uint64)
    u = (key >> np.uint64(32)) & np.uint64(0xFFFFFFFF)
    neg = (u & np.uint64(0x80000000)) == 0
    bits = np.where(neg, ~u & np.uint64(0xFFFFFFFF), u & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    return bits.view(F32).astype(np.float64), (np.uint64(0x7FFFFFFF) - (key & np.uint64(0xFFFFFFFF))).astype(np.int64)


def key_encode(val, idx):
    """the inverse, for the host test (and its defect: the LAST of two equal maxima)"""
    bits = np.asarray(val, F32).view(np.uint32).astype(np.uint64)
    u = np.where(bits & np.uint64(0x80000000), ~bits & np.uint64(0xFFFFFFFF), bits | np.uint64(0x80000000))
    return ((u << np.uint64(32)) | (np.uint64(0x7FFFFFFF) - np.asarray(idx).astype(np.uint64))).astype(np.uint64)


# ======================================================================================================================
# 3. BatchNorm (rsis_blk_bn_fwd / rsis_blk_bn_bwd)
# ======================================================================================================================
BLK_BN_BLOCK_MAX, BN_MINCELLS = 4096, 1024


def bn_plan(B, C, H, W):
    """rsis_l_blk_bn_fwd / _bwd (blk_norm.hip) restated: the kernel family, NPT or the splits, and the shape of the only fp32 accumulation of
    a launch, a wave's (block_sum16*): every thread adds its p cells one after the other (cells t, t + T, t + 2 T, ... of its block of T
    threads), the 64 lanes are folded by 6 fp32 shuffle steps (a balanced tree), and the waves of a block and the splits meet in double.
      block kernel  : T = 512 threads x p = NPT cells, one block per channel block   -> wave_cells = 64 NPT
      two-pass      : a split of `per` cells on T = 256 threads, p = per / 256        -> wave_cells = per / 4
    wave_sums() below is that order in numpy -- the host model of the sums.  `chain` = wave_cells is the length of ONE sequential fp32
    chain over the cells that meet in fp32 (chain_sums): on N(16, 2) data it is no yardstick either way -- x^2 of a bf16 x below 16 is
    a multiple of 2^-8, so a chain is EXACT until its partial sum passes 2^16 (250 cells) and loses a bit per addition after that:
    a chain of 512 cells shows 6.6e-5 relative on rstd at N = 4096 where the fold's tree has 9e-7 (measured), one of 55 cells shows
    5e-8 (NOTES.md (93))."""
    N, Cb = B * H * W, C // 8
    if N <= BLK_BN_BLOCK_MAX:
        npt = 4 if N <= 2048 else 8
        return dict(N=N, kernel="block", NPT=npt, S=1, per=N, wave_cells=64 * npt, chain=64 * npt, block_cells=N)
    s = max(1, 2048 // Cb)
    s = max(1, min(s, (N + BN_MINCELLS - 1) // BN_MINCELLS, 64))
    per = (N + s - 1) // s
    per = (per + 255) // 256 * 256
    S = (N + per - 1) // per
    return dict(N=N, kernel="two-pass", NPT=0, S=S, per=per, wave_cells=per // 4, chain=per // 4, block_cells=per, last=N - (S - 1) * per)


def _bn(B, C, H, W, why, **expect):
    return dict(B=B, C=C, H=H, W=W, why=why, expect=expect)


BN_CASES = [
    _bn(2, 8, 1, 1, "two cells: dx is pure cancellation", kernel="block", NPT=4),
    _bn(3, 24, 5, 9, "135 cells, three channel blocks, ragged", kernel="block", NPT=4),
    _bn(8, 8, 16, 16, "2048: the last N of NPT 4, every thread holds 4 cells", kernel="block", NPT=4),
    _bn(3, 8, 683, 1, "2049: the first N of NPT 8, one thread holds a fifth cell; HW = 683 divides no power of two", kernel="block", NPT=8),
    _bn(16, 8, 16, 16, "4096: the last N of the block kernel, every thread holds 8 cells", kernel="block", NPT=8),
    _bn(1, 8, 17, 241, "4097: the first two-pass N; 5 splits of 1024, the last one holds ONE cell", kernel="two-pass", S=5, per=1024, last=1),
    _bn(32, 24, 14, 14, "6272: 7 splits of 1024 with 128 cells in the last", kernel="two-pass", S=7, per=1024, last=128),
    _bn(8, 64, 56, 56, "25088: 25 splits: the apply pass adds more than 16 partials per channel (two trips of its 16-lane loop)", kernel="two-pass", S=25, per=1024, last=512),
    _bn(6, 8, 112, 112, "75264: the 64-split cap: 59 splits of 1280", kernel="two-pass", S=59, per=1280, last=1024),
]
BN_EVAL_SHAPES = [BN_CASES[4], BN_CASES[5]]          # eval mode at the block / two-pass boundary (always the apply kernel)
BN_EXACT_SETS = {"pm3": (-3, 3), "far": (13, 19)}    # integer x; `far`: a mean of ~8 standard deviations, where E[x^2] - m^2 cancels
BN_NORMAL_SETS = {"n05": 0.5, "n16": 16.0}           # bf16-valued N(mean, 2)
BN_EPS, BN_MOMENTUM = float(F32(1e-5)), float(F32(0.1))      # the fp32 values the entry points receive: the float64 references use these
R_RSQRT = 1.0                         # rsqrtf in ulp: ceil of the worst error probed on the device at the cases' own arguments, 0.70 (NOTES.md (93))
K_RSTD_ULP = 1.0 + (np.ceil(R_RSQRT) + 1.0)          # save_rstd: one ulp for the fp32 argument (float)var + eps, ceil(R) + 1 for rsqrtf
M_BN = 2.0                            # sums: twice the worst measured err_gpu / err_host, 2 x 1.000; must stay <= 4 (NOTES.md (93))


def bn_id(c):
    return "b%d_c%d_%dx%d" % (c["B"], c["C"], c["H"], c["W"])


def bn_seed(c):
    return (c["B"] * 7 + c["C"] * 131 + c["H"] * 1009 + c["W"] * 53) % 100003 + 2000


def _bf16_normal(rng, shape, mean=0.0, std=1.0):
    return bf16_rne64(rng.standard_normal(shape) * std + mean)


def bn_inputs(c, regime):
    """x, residual, dy (bf16-valued float64, NCHW), gamma / beta / running statistics (fp32-valued), integer prefills of dgamma / dbeta"""
    B, C, H, W = (c[k] for k in ("B", "C", "H", "W"))
    rng = _rng(bn_seed(c) + sorted(list(BN_EXACT_SETS) + list(BN_NORMAL_SETS)).index(regime))
    shape = (B, C, H, W)
    if regime in BN_EXACT_SETS:
        lo, hi = BN_EXACT_SETS[regime]
        x, dy, res = _ints(rng, shape, lo, hi), _ints(rng, shape), _ints(rng, shape)
    else:
        x, dy, res = _bf16_normal(rng, shape, BN_NORMAL_SETS[regime], 2.0), _bf16_normal(rng, shape), _bf16_normal(rng, shape)
    f = lambda a: a.astype(F32).astype(np.float64)
    return dict(x=x, dy=dy, res=res, gamma=f(rng.random(C) + 0.5), beta=f(rng.standard_normal(C) * 0.3), rm=f(rng.standard_normal(C) * 0.1),
                rv=f(rng.random(C) + 0.5), dg0=_ints(rng, (C,), -5, 5), db0=_ints(rng, (C,), -5, 5))


def bn_stats64(x, drop_cell=None, n_minus_1=False):
    """batch mean / biased variance / rstd / unbiased variance per channel in float64.  Defect switches for the host test: drop_cell = n
    leaves cell n of the flattened (b, h, w) order out of both sums (a split boundary that loses a cell); n_minus_1 divides by N - 1."""
    B, C, H, W = x.shape
    xs = x.transpose(1, 0, 2, 3).reshape(C, -1)
    N = xs.shape[1]
    s, q = xs.sum(1), (xs * xs).sum(1)
    if drop_cell is not None:
        s, q = s - xs[:, drop_cell], q - xs[:, drop_cell] ** 2
    n = N - 1 if n_minus_1 else N
    m = s / n
    var = np.maximum(q / n - m * m, 0.0)
    return dict(N=N, mean=m, var=var, rstd=1.0 / np.sqrt(var + BN_EPS), unb=var * N / (N - 1) if N > 1 else var)


def bn_fwd64(d, relu, res, st=None):
    """y (float64, unrounded) and its pre-activation; running statistics after the update"""
    st = st or bn_stats64(d["x"])
    v = lambda a: a[None, :, None, None]
    pre = (d["x"] - v(st["mean"])) * v(st["rstd"]) * v(d["gamma"]) + v(d["beta"]) + (d["res"] if res else 0.0)
    return dict(st=st, pre=pre, y=np.maximum(pre, 0.0) if relu else pre, rm=(1 - BN_MOMENTUM) * d["rm"] + BN_MOMENTUM * st["mean"],
                rv=(1 - BN_MOMENTUM) * d["rv"] + BN_MOMENTUM * st["unb"])


def bn_bwd64(d, st, mask):
    """g = dy * mask;  dbeta = sum g, dgamma = sum g xhat, dx = gamma rstd (g - mean(g) - xhat mean(g xhat)), dres = g"""
    v = lambda a: a[None, :, None, None]
    g = d["dy"] * mask
    xh = (d["x"] - v(st["mean"])) * v(st["rstd"])
    db, dg = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    c1, c2 = db / st["N"], dg / st["N"]
    return dict(g=g, xh=xh, dbeta=db, dgamma=dg, c1=c1, c2=c2, dx=v(d["gamma"] * st["rstd"]) * (g - v(c1) - xh * v(c2)))


def chain_sums(a, chain):
    """the sequential yardstick (bn_plan says why it is not the model): a [C][N] fp32 -- consecutive runs of `chain` cells, each ONE sequential
    fp32 chain, the runs added in float64"""
    a = np.asarray(a, F32)
    C, N = a.shape
    pad = (-N) % chain
    a = np.concatenate([a, np.zeros((C, pad), F32)], 1).reshape(C, -1, chain)
    return np.cumsum(a, axis=2, dtype=F32)[:, :, -1].astype(np.float64).sum(1)


def wave_sums(a, plan, b=None):
    """host model of the kernels' sums, in their own order (bn_plan): per channel the sum of a[C][N] (or of a * b, each product fused into
    its addition as the compiler contracts `acc += g * xh`) -- per-thread sequential fp32, the 64-lane xor fold in fp32, the rest in double"""
    a = np.asarray(a, F32)
    C, N = a.shape
    if plan["kernel"] == "block":
        T, p, blocks = 512, plan["NPT"], 1
    else:
        T, p, blocks = 256, plan["per"] // 256, plan["S"]
    pad = blocks * T * p - N
    shape = (C, blocks, p, T)
    a = np.concatenate([a, np.zeros((C, pad), F32)], 1).reshape(shape)
    if b is not None:
        b = np.concatenate([np.asarray(b, F32), np.zeros((C, pad), F32)], 1).reshape(shape)
    acc = np.zeros((C, blocks, T), F32)
    for j in range(p):
        if b is None:
            acc = acc + a[:, :, j]
        else:
            acc = (acc.astype(np.float64) + a[:, :, j].astype(np.float64) * b[:, :, j].astype(np.float64)).astype(F32)
    v = acc.reshape(C, blocks, T // 64, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    assert v.dtype == F32
    return v[..., 0].astype(np.float64).sum((1, 2))


def bn_model32(d, c, relu, res, mask=None, store=bf16_rne64, drop_cell=None, n_minus_1=False, mask_defect=False):
    """numpy fp32 model of the forward and backward kernels' arithmetic (fp32 products and additions, fused multiply-adds as the compiler
    contracts them are modelled as the float64 product rounded once; sums by wave_sums, the launch's own order).  The defect switches serve
    the host test.  Returns fp32 statistics, the stored y / dx / dres (bf16 values as float64) and the parameter gradients."""
    plan = bn_plan(c["B"], c["C"], c["H"], c["W"])
    x = d["x"]
    B, C, H, W = x.shape
    N = plan["N"]
    flat = lambda a: a.transpose(1, 0, 2, 3).reshape(C, -1)
    xs = flat(x).astype(F32)
    s, q = wave_sums(xs, plan), wave_sums(xs, plan, xs)
    if drop_cell is not None:
        s, q = s - flat(x)[:, drop_cell], q - flat(x)[:, drop_cell] ** 2
    n = N - 1 if n_minus_1 else N
    m = s / n
    var = np.maximum(q / n - m * m, 0.0)
    mean = m.astype(F32)
    rstd = (F32(1) / np.sqrt((var.astype(F32) + F32(BN_EPS)).astype(np.float64))).astype(F32)
    unb = (var * N / (N - 1) if N > 1 else var).astype(F32)
    mom = F32(BN_MOMENTUM)
    rm = ((F32(1) - mom) * d["rm"].astype(F32) + mom * mean).astype(F32)
    rv = ((F32(1) - mom) * d["rv"].astype(F32) + mom * unb).astype(F32)
    sc = (d["gamma"].astype(F32) * rstd).astype(F32)
    sh = (d["beta"] - mean.astype(np.float64) * sc.astype(np.float64)).astype(F32)
    v = lambda a: np.asarray(a, np.float64)[None, :, None, None]
    pre = (x * v(sc) + v(sh)).astype(F32)
    if res:
        pre = (pre + d["res"].astype(F32)).astype(F32)
    yv = np.maximum(pre, F32(0)) if relu else pre
    y = store(yv.astype(np.float64))
    # rsqrtf is a hardware unit within ceil(R) ulp of the root: the model carries that as the three values rstd - 1 ulp, rstd, rstd + 1 ulp
    # (rstd_var); the error of a quantity that depends on rstd is the largest over the three
    nudge = lambda k: rstd if k == 0 else np.nextafter(rstd, F32(np.inf) if k > 0 else F32(0)).astype(F32)
    rstd_var = [nudge(k) for k in range(-int(np.ceil(R_RSQRT)), int(np.ceil(R_RSQRT)) + 1)]
    out = dict(mean=mean, rstd=rstd, rstd_var=rstd_var, rm=rm, rv=rv, y=y, y32=yv.astype(np.float64), pre32=pre)
    if d.get("dy") is None:
        return out
    if mask is None:
        mask = (y > 0) if relu else np.ones_like(y, bool)
        if mask_defect and relu:      # the mask taken from the UNROUNDED value, with the sign flipped at the smallest positive result
            pos = np.where(pre > 0, pre, np.inf)
            mask = pre > 0
            mask.reshape(-1)[int(np.argmin(pos))] = False
    g = (d["dy"] * mask).astype(F32)
    xh = ((x.astype(F32) - v(mean).astype(F32)) * v(rstd).astype(F32)).astype(F32)
    db, dg = wave_sums(flat(g), plan), wave_sums(flat(g), plan, flat(xh))
    c1, c2 = (db / N).astype(F32), (dg / N).astype(F32)
    t = (g - v(c1).astype(F32)).astype(F32)
    t = (t.astype(np.float64) - xh.astype(np.float64) * v(c2)).astype(F32)
    gr = (d["gamma"].astype(F32) * rstd).astype(F32)
    dx = store((v(gr).astype(F32) * t).astype(F32).astype(np.float64))
    dx32 = (v(gr).astype(F32) * t).astype(F32).astype(np.float64)
    dg_var = [dg.astype(F32) if r is rstd else
              wave_sums(flat(g), plan, flat(((x.astype(F32) - v(mean).astype(F32)) * v(r).astype(F32)).astype(F32))).astype(F32) for r in rstd_var]
    out.update(dbeta=db.astype(F32), dgamma=dg.astype(F32), dgamma_var=dg_var, dx=dx, dx32=dx32, dres=store(g.astype(np.float64)), mask=mask)
    return out


# ---- derived deltas of the normal regime (in units of U24 = 2^-24, one fp32 rounding; an R-ulp function error is 2 R of them) ----
# y = x sc + sh (+ res), sc = gamma rstd, sh = beta - mean sc.  sc is formed ONCE and enters both terms, so its error multiplies
# (x - mean) sc = pre - beta - res, not the large terms x sc and mean sc that cancel:
#   rstd   (float)var 1, + eps 1 -> halved by the root: 1;  rsqrtf 2 R;  sc: + 1 for the product  -> (2 + 2 R) |pre - beta - res|
#   sh     one rounding (fused) of |sh| <= |beta| + |mean sc|                                    -> |mean sc| + |beta|
#          (the rounding (float)m is part of save_mean's own error: it enters through e_mean below, and eval mode has none)
#   x sc + sh: one rounding (fused) of pre - res;   + res: one rounding of pre                      -> |pre - res| (+ |pre|)
K_SC = 2.0 + 2.0 * np.ceil(R_RSQRT)
# the statistics' own errors enter through dy / dmean = -sc and dy / drstd = (x - mean) gamma, with the sums' bars (bn_delta_y).
#
# dx = gr (g - c1 - xh c2), gr = gamma rstd (K_SC as sc), xh = (x - mean) rstd, c1 / c2 = (float) of a double (1/2 each):
#   xh     the subtraction 1, rstd 1 + 2 R, the product 1 ((float)m: through e_mean)                -> (3 + 2 R) |xh|
#   t      g - c1: 1 on |g - c1| <= |g| + |c1|;  t - xh c2 (fused): 1 on |dx| / gr;  c2: 1/2 |xh c2|
#   dx     gr: K_SC, the last product 1, t's fused rounding 1                                      -> (K_SC + 2) |dx|
# the statistics' and the sums' bars enter with the sensitivities written out in bn_delta_dx.


def bn_delta_y(d, f, res, e_mean, e_rstd_rel):
    """e_mean: the bar of save_mean (absolute); e_rstd_rel: that of save_rstd relative to rstd.  dy / dmean = -sc, dy / drstd = (x - mean) gamma"""
    st = f["st"]
    v = lambda a: a[None, :, None, None]
    sc = np.abs(d["gamma"] * st["rstd"])
    r = d["res"] if res else 0.0
    aff = np.abs(f["pre"] - v(d["beta"]) - r)                                   # |(x - mean) sc|
    mag = K_SC * aff + v(np.abs(st["mean"]) * sc + np.abs(d["beta"])) + np.abs(f["pre"] - r) + (np.abs(f["pre"]) if res else 0.0)
    return U24 * mag + v(sc) * e_mean + aff * e_rstd_rel


def bn_delta_dx(d, st, b, e_mean, e_rstd_rel, e_db, e_dg):
    """statistics: d gr = gr e_r, d xh = -rstd d mean + xh e_r;  sums: d c1 = e_db / N, d c2 = e_dg / N"""
    v = lambda a: a[None, :, None, None]
    gr = np.abs(d["gamma"] * st["rstd"])
    N = st["N"]
    c1, c2, xh = np.abs(b["c1"]), np.abs(b["c2"]), np.abs(b["xh"])
    d_xh = (3.0 + 2.0 * np.ceil(R_RSQRT)) * xh
    mag = v(gr) * (np.abs(b["g"]) + v(1.5 * c1) + v(c2) * (d_xh + 0.5 * xh)) + (K_SC + 2.0) * np.abs(b["dx"])
    stat = np.abs(b["dx"]) * e_rstd_rel + v(gr * c2) * (v(st["rstd"]) * e_mean + xh * e_rstd_rel)
    return U24 * mag + stat + v(gr) * (e_db / N + xh * e_dg / N)


def bn_sum_errors(model, ref_f, ref_b=None):
    """err_host: largest error per sum quantity over the channels: mean (absolute), rstd (relative to rstd), dbeta, dgamma (absolute); rstd and
    dgamma (through xhat) over the model's three values of rsqrtf (bn_model32: rstd_var)"""
    st = ref_f["st"]
    e = dict(mean=float(np.abs(model["mean"].astype(np.float64) - st["mean"]).max()),
             rstd=max(float((np.abs(r.astype(np.float64) - st["rstd"]) / st["rstd"]).max()) for r in model["rstd_var"]))
    if ref_b is not None:
        e["dbeta"] = float(np.abs(model["dbeta"].astype(np.float64) - ref_b["dbeta"]).max())
        e["dgamma"] = max(float(np.abs(g.astype(np.float64) - ref_b["dgamma"]).max()) for g in model["dgamma_var"])
    return e


def bn_tie_data(shape=(2, 16, 9, 31)):
    """exact-regime store check of the BatchNorm kernels (eval mode: gamma = 1, running_var = 1, eps = 0, running_mean = 0, beta = 1/2):
    x integers in 128..255 (bf16 values), so y = x + 1/2 is exact in fp32 and EVERY output is a tie between two bf16 values"""
    rng = _rng(77)
    x = _ints(rng, shape, 128, 255)
    C = shape[1]
    return dict(x=x, gamma=np.ones(C), beta=np.full(C, 0.5), rm=np.zeros(C), rv=np.ones(C), y=x + 0.5)


def clear_of_zero(pre, relu):
    """the existing rule of test_gpu_blk.py: elements whose float64 pre-activation is clear of the ReLU's kink"""
    return (np.abs(pre) > 2.0 ** -7 * (np.abs(pre) + 1)) if relu else np.ones_like(pre, bool)


# ======================================================================================================================
# 4. layout helpers
# ======================================================================================================================
def from_nchw_specials():
    """fp32 values for rsis_blk_from_nchw: ties, both fp32 neighbours of a tie, values next to a binade boundary, +-0, +-inf, NaN, fp32
    denormals, the largest finite fp32 and the values around the largest finite bf16"""
    v = []
    for e in (-126, -20, -1, 0, 1, 7, 100, 126):
        for m in (0, 1, 2, 63, 126, 127):
            base = np.ldexp(1.0 + m / 128.0, e)
            ulp = np.ldexp(1.0, e - 7)
            tie = base + ulp / 2
            f32ulp = np.ldexp(1.0, e - 23)
            v += [base, tie, tie - f32ulp, tie + f32ulp, base + f32ulp, base + ulp - f32ulp]
    v += [np.ldexp(1.0, -149), np.ldexp(1.0, -134), np.ldexp(3.0, -134), np.ldexp(1.0, -133), np.ldexp(1.5, -133), np.ldexp(2.5, -133),
          np.ldexp(1.0, -127), float(np.finfo(F32).max), _BF16_MAX, _BF16_MAX + np.ldexp(1.0, 119), _BF16_MAX + np.ldexp(1.0, 119) - np.ldexp(1.0, 104),
          1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 - 2.0 ** -9, 1.0 - 3 * 2.0 ** -9, 0.0]
    v = np.array(v, np.float64)
    assert np.array_equal(v.astype(F32).astype(np.float64), v), "every special is an fp32 value"
    v = np.concatenate([v, -v, [np.inf, -np.inf, np.nan]])
    return v


COPY_MAPS = [(7, 7), (9, 14), (8, 8)]
COPY_STRIDES = [2, 3]
COPY_B, COPY_C = 3, 40                # 3 x 5 channel blocks x 49..126 cells: 735..1890 cells, several 256-thread blocks
