"""Case tables of the fp32 resize and pooling tests (test_gpu_resample.py on the GPU, test_resample_host.py on the host): plain data, the
launch rules of rsis_amd/csrc/pointwise.hip restated as small pure functions in fp32 arithmetic, and the float64 references.  Nothing here
touches the GPU.

Every case is a dict with a `why` (the edge it is the smallest instance of) and the path the restated rule must give for it.  The cases
at the edge of a gate are FOUND with the restated rules (find_*), not written down by hand.  If a rule of pointwise.hip is retuned,
test_resample_host.py fails: update the rule here and the cases that sat at its edges."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
U = 2.0 ** -24                  # unit roundoff of fp32
UK = 6                          # candidate outputs per input index of upsample_bwd_kernel
GRID_CAP = 256 * 16             # ew_grid: blocks of 256 threads
TWO20 = 1 << 20                 # GRID_CAP * 256: more work items than this = a second trip of a grid-stride loop
ROBUST = 1e-4                   # a case counts as on one side of a gate only if float64 arithmetic puts it there by this much


def cdiv(a, b):
    return (a + b - 1) // b


def ew_grid(total):
    return int(max(1, min(cdiv(total, 256), GRID_CAP)))


# ---------------------------------------------------------------- ac_scale / ac_coord (common.h)
def ac_scale(n_in, n_out):
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)


def ac_coord(o, scale, n_in):
    """(i0, i1, l1) of the outputs o (array): src = scale * o ROUNDED to fp32 gives i0 = (int)src, clamped; l1 = fma(scale, o, -i0), one
    rounding of the exact scale * o - i0 (exact in float64: a 24-bit by 24-bit product less an integer below it)"""
    o = np.asarray(o, np.int64)
    src = F32(scale) * o.astype(F32)
    assert src.dtype == F32
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (np.float64(F32(scale)) * o.astype(np.float64) - i0).astype(F32)
    return i0, i1, l1


# ---------------------------------------------------------------- rsis_l_upsample_fwd, restated
LDS_TILES = {"lds16x128": dict(toh=16, tow=128, rh=12, rq=18), "lds32x64": dict(toh=32, tow=64, rh=20, rq=12)}
_GATE = {"lds16x128": (15, 12, 127, 72), "lds32x64": (31, 20, 63, 48)}      # fh * a + 3 <= b, fw * c + 6 <= d


def lds_gate_sides(which, Hi, Wi, Ho, Wo, dt=F32):
    """(h side, w side) of one LDS gate, each lhs - rhs in dtype dt: <= 0 passes"""
    a, b, c, d = _GATE[which]
    fh, fw = dt(ac_scale(Hi, Ho)), dt(ac_scale(Wi, Wo))
    return fh * dt(a) + dt(3) - dt(b), fw * dt(c) + dt(6) - dt(d)


def lds_gate(which, Hi, Wi, Ho, Wo):
    t = LDS_TILES[which]
    sh, sw = lds_gate_sides(which, Hi, Wi, Ho, Wo)
    return Ho >= t["toh"] and Wo >= t["tow"] and sh <= 0 and sw <= 0


def wq_shift(Wq):
    """index mode of upsample_fwd_v4_kernel: log2(Wq) for a power of two <= 256, -2 for any other Wq <= 256, -1 above"""
    if Wq <= 256 and (Wq & (Wq - 1)) == 0:
        return Wq.bit_length() - 1
    return -2 if Wq <= 256 else -1


def upsample_fwd_path(BC, Hi, Wi, Ho, Wo):
    al = Wo % 4 == 0 and Wi % 4 == 0
    for which in ("lds16x128", "lds32x64"):
        t = LDS_TILES[which]
        if al and lds_gate(which, Hi, Wi, Ho, Wo) and BC * cdiv(Wo, t["tow"]) * cdiv(Ho, t["toh"]) < (1 << 31):
            return which
    if Wo % 4 == 0 and BC * Ho < (1 << 31):
        return "v4[%d]" % wq_shift(Wo // 4)
    return "scalar"


def lds_tile_origins(which, Hi, Wi, Ho, Wo):
    """[(oh0, ow0, h_lo, w_lo)] of every tile of an LDS launch"""
    t = LDS_TILES[which]
    fh, fw = ac_scale(Hi, Ho), ac_scale(Wi, Wo)
    out = []
    for oh0 in range(0, Ho, t["toh"]):
        for ow0 in range(0, Wo, t["tow"]):
            out.append((oh0, ow0, int(ac_coord([oh0], fh, Hi)[0][0]), int(ac_coord([ow0], fw, Wi)[0][0])))
    return out


def _fwd_gate_robust(which, Hi, Wi, Ho, Wo, want):
    s64 = lds_gate_sides(which, Hi, Wi, Ho, Wo, np.float64)
    return lds_gate(which, Hi, Wi, Ho, Wo) == want and all(abs(s) > ROBUST for s in s64)


@functools.lru_cache(None)
def find_fwd_gate_edge(which):
    """(Hi, Wi, Ho, Wo): per axis the LARGEST scale the gate lets through whose next step (Hi + 1, Wi + 4) it refuses, with a tile (not
    the first) whose first source column is 3 mod 4 -- the staged patch then starts three columns before the first one used"""
    t = LDS_TILES[which]
    best_h = best_w = None
    for Ho in range(2 * t["toh"] + 1, 4 * t["toh"]):                  # odd heights too: a partial last tile
        for Hi in range(2, Ho):
            ok = lds_gate_sides(which, Hi, 4, Ho, 1 << 20, np.float64)[0] < -ROBUST and lds_gate_sides(which, Hi, 4, Ho, 1 << 20)[0] <= 0
            bad = lds_gate_sides(which, Hi + 1, 4, Ho, 1 << 20, np.float64)[0] > ROBUST and lds_gate_sides(which, Hi + 1, 4, Ho, 1 << 20)[0] > 0
            if ok and bad and (best_h is None or ac_scale(Hi, Ho) > ac_scale(*best_h)):
                best_h = (Hi, Ho)
    for Wo in range(t["tow"] + 4, 3 * t["tow"] + 1, 4):
        for Wi in range(4, Wo, 4):
            ok = lds_gate_sides(which, 2, Wi, 1 << 20, Wo, np.float64)[1] < -ROBUST and lds_gate_sides(which, 2, Wi, 1 << 20, Wo)[1] <= 0
            bad = lds_gate_sides(which, 2, Wi + 4, 1 << 20, Wo, np.float64)[1] > ROBUST and lds_gate_sides(which, 2, Wi + 4, 1 << 20, Wo)[1] > 0
            if not (ok and bad):
                continue
            w_los = [int(ac_coord([ow0], ac_scale(Wi, Wo), Wi)[0][0]) for ow0 in range(t["tow"], Wo, t["tow"])]
            if any(w % 4 == 3 for w in w_los) and (best_w is None or ac_scale(Wi, Wo) > ac_scale(*best_w)):
                best_w = (Wi, Wo)
    return best_h[0], best_w[0], best_h[1], best_w[1]


def _u(why, path, BC, Hi, Wi, Ho, Wo, **kw):
    d = dict(why=why, path=path, BC=BC, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo)
    d.update(kw)
    return d


def case_id(c):
    if "HW" in c:
        return "%s_BC%d_HW%d" % (c["kind"], c["BC"], c["HW"])
    if "H" in c:
        return "BC%d_%dx%d" % (c["BC"], c["H"], c["W"])
    return "BC%d_%dx%d_to_%dx%d" % (c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"])


def case_seed(c):
    return 4000 + 7 * (sum(map(ord, case_id(c))) % 991)


def _up_fwd_cases():
    e16, e32 = find_fwd_gate_edge("lds16x128"), find_fwd_gate_edge("lds32x64")
    return [
        _u("16 x 128 LDS kernel, exactly one tile per plane", "lds16x128", 2, 8, 64, 16, 128),
        _u("16 x 128 LDS kernel, two tiles per axis, the last ones partial both ways", "lds16x128", 3, 10, 72, 20, 144),
        _u("16 x 128 LDS kernel at the largest fh and fw its gate passes, a tile with w_lo % 4 == 3: the patch at its full 12 x 72", "lds16x128",
           2, e16[0], e16[1], e16[2], e16[3]),
        _u("16 x 128 LDS kernel at a tiny scale (8 -> 256, the inference-time resize): every tile reads two source columns", "lds16x128",
           2, 8, 8, 256, 256),
        _u("32 x 64 LDS kernel, exactly one tile per plane", "lds32x64", 2, 16, 32, 32, 64),
        _u("32 x 64 LDS kernel, two tiles per axis, the last ones partial both ways", "lds32x64", 3, 20, 36, 40, 72),
        _u("32 x 64 LDS kernel on the 56 -> 112 level of the 224^2 pyramid (Wo < 128)", "lds32x64", 2, 56, 56, 112, 112),
        _u("32 x 64 LDS kernel at the largest fh and fw its gate passes, a tile with w_lo % 4 == 3: the patch at its full 20 x 48", "lds32x64",
           2, e32[0], e32[1], e32[2], e32[3]),
        _u("one row more than the 16 x 128 gate's fh allows (the 32 x 64 gate's fh is tighter still) -> v4", "v4[%d]" % wq_shift(e16[3] // 4),
           2, e16[0] + 1, e16[1], e16[2], e16[3]),
        _u("one float4 more than the 16 x 128 gate's fw allows, Ho < 32 so that the 32 x 64 kernel cannot take it -> v4",
           "v4[%d]" % wq_shift(e16[3] // 4), 2, 10, e16[1] + 4, 20, e16[3]),
        _u("one row more than the 32 x 64 gate's fh allows -> v4", "v4[%d]" % wq_shift(e32[3] // 4), 2, e32[0] + 1, e32[1], e32[2], e32[3]),
        _u("one float4 more than the 32 x 64 gate's fw allows -> v4", "v4[%d]" % wq_shift(e32[3] // 4), 2, e32[0], e32[1] + 4, e32[2], e32[3]),
        _u("v4, shift 0 (Wo = 4: a block spans 256 rows), 350 rows: a tail block", "v4[0]", 70, 3, 2, 5, 4),
        _u("v4, shift 3 (Wo = 32: a block spans 32 rows), 21 rows: less than one block", "v4[3]", 3, 4, 16, 7, 32),
        _u("v4, shift 8 (Wo = 1024: a block is one row), Ho < 16 keeps the LDS kernels out", "v4[8]", 2, 4, 512, 8, 1024),
        _u("v4, shift -2 (Wq = 7, the 14 -> 28 level): the (row, float4) space walked flat, last block partial", "v4[-2]", 3, 14, 14, 28, 28),
        _u("v4, shift -2 (Wq = 33), a row straddles two blocks", "v4[-2]", 2, 8, 66, 15, 132),
        _u("v4, shift -1 (Wq = 257: blockIdx.y walks the row, its second block has ONE live thread), Hi = Ho = 2", "v4[-1]", 3, 2, 514, 2, 1028),
        _u("scalar kernel (Wo % 4 != 0) with more than 2^20 outputs: the second trip of its grid-stride loop", "scalar", 11, 155, 155, 310, 310),
        _u("scalar kernel, odd sizes", "scalar", 6, 4, 5, 7, 9),
        _u("scalar kernel, a 1 x 1 input (scale 0)", "scalar", 4, 1, 1, 3, 3),
        _u("identity resize on the scalar kernel (scale 1: the input's bits)", "scalar", 3, 5, 7, 5, 7, identity=True),
        _u("identity resize on the v4 kernel (scale 1: the input's bits)", "v4[1]", 2, 8, 8, 8, 8, identity=True),
    ]


# ---------------------------------------------------------------- rsis_l_upsample_bwd, restated
def upsample_bwd_path(BC, Hi, Wi, Ho, Wo):
    """dict(kernel = tiled16 | tiled32 | generic, ...): the tiled kernel needs min(scale) >= 0.4 (2 / smin + 1 <= UK) and its dy region to
    fit RM = 44 / 80 staged rows and columns ((ut - 1) / smin + UK + 3 <= RM); any scale ABOVE that runs it too, down-sampling included"""
    sh, sw = ac_scale(Hi, Ho), ac_scale(Wi, Wo)
    smin = min(sh, sw)
    tiled = bool(smin > 0 and F32(2) / smin + F32(1) <= UK)
    ut = 32 if (Hi > 16 or Wi > 16) else 16
    rm = 80 if ut == 32 else 44
    fits = tiled and bool((F32(ut - 1) / smin + F32(UK)) + F32(3) <= rm)
    if not fits:
        return dict(kernel="generic", grid=ew_grid(BC * Hi * Wi), items=BC * Hi * Wi)
    tiles_x, tiles_y = cdiv(Wi, ut), cdiv(Hi, ut)
    ppb = min(16, max(1, BC * tiles_x * tiles_y // 2048))
    return dict(kernel="tiled%d" % ut, ut=ut, rm=rm, tiles_x=tiles_x, tiles_y=tiles_y, ppb=ppb, vec=int(Wo % 4 == 0),
                blocks=cdiv(BC, ppb) * tiles_x * tiles_y)


def _bwd_fit_margin(n_in, n_out, ut):
    """float64 (tiled side, fits side) of a square map: <= 0 passes"""
    s = float(n_in - 1) / float(n_out - 1)
    return 2.0 / s + 1.0 - UK, (ut - 1) / s + UK + 3 - (80 if ut == 32 else 44)


@functools.lru_cache(None)
def find_bwd_fit_edge(ut):
    """(n, out_fit, out_generic): the square n x n map with the SMALLEST scale the tiled kernel of this ut still takes, and the next
    output size, which the generic kernel gets"""
    best = None
    for n in (range(4, 17) if ut == 16 else range(17, 41)):
        for out in range(n, 3 * n):
            ok = upsample_bwd_path(1, n, n, out, out)["kernel"] == "tiled%d" % ut and max(_bwd_fit_margin(n, out, ut)) < -ROBUST
            bad = upsample_bwd_path(1, n, n, out + 1, out + 1)["kernel"] == "generic" and max(_bwd_fit_margin(n, out + 1, ut)) > ROBUST
            if ok and bad and (best is None or ac_scale(n, out) < ac_scale(best[0], best[1])):
                best = (n, out)
    return best[0], best[1], best[1] + 1


def _up_bwd_cases():
    f16, f32 = find_bwd_fit_edge(16), find_bwd_fit_edge(32)
    return [
        _u("ut = 16, float4 staging", "tiled16", 6, 8, 8, 16, 16, ppb=1, vec=1),
        _u("ut = 16, Wo % 4 != 0: scalar staging", "tiled16", 6, 4, 5, 7, 9, ppb=1, vec=0),
        _u("ut = 32 with one dimension <= 16: most of the tile's rows lie beyond the map", "tiled32", 4, 8, 40, 16, 80, ppb=1, vec=1),
        _u("ut = 32, two tiles per axis with a partial last tile", "tiled32", 3, 40, 36, 80, 72, ppb=1, vec=1),
        _u("ut = 32, two tiles down, scalar staging (Wo % 4 != 0)", "tiled32", 3, 33, 20, 66, 41, ppb=1, vec=0),
        _u("ut = 16 at the smallest scale that still fits its 44-wide region", "tiled16", 3, f16[0], f16[0], f16[1], f16[1], ppb=1),
        _u("ut = 16, one output more: the region no longer fits -> generic", "generic", 3, f16[0], f16[0], f16[2], f16[2]),
        _u("ut = 32 at the smallest scale that still fits its 80-wide region", "tiled32", 3, f32[0], f32[0], f32[1], f32[1], ppb=1),
        _u("ut = 32, one output more: the region no longer fits -> generic", "generic", 3, f32[0], f32[0], f32[2], f32[2]),
        _u("planes_per_block = 2 with an odd BC: the last block's plane loop stops at bc >= BC", "tiled16", 4099, 8, 8, 16, 16, ppb=2, vec=1),
        _u("planes_per_block = 16 (the step's value) with a BC that 16 does not divide.  4 -> 8 is scale 3/7, EXACTLY on the fits gate of "
           "ut = 16 (15 / (3/7) + 9 = 44): the launcher's fp32 arithmetic passes it, and the step runs this level", "tiled16", 32773, 4, 4, 8, 8,
           ppb=16, vec=1, on_gate=True),
        _u("planes_per_block = 2 with two tiles per plane: bc0 from blockIdx / (tiles_x * tiles_y)", "tiled32", 2049, 33, 5, 66, 8, ppb=2, vec=1),
        _u("generic kernel at scale 7 / 31 = 0.23 (8 -> 32): a nine-output candidate window per axis", "generic", 3, 8, 8, 32, 32),
        _u("generic kernel, down-sampling by 2.4 in h (40 -> 17) next to 0.23 in w", "generic", 3, 40, 8, 17, 32),
        _u("generic kernel with more than 2^20 inputs: the second trip of its grid-stride loop", "generic", 3300, 40, 8, 17, 32),
        _u("generic kernel, a 1 x 1 input (scale 0: the window is the whole map)", "generic", 4, 1, 1, 3, 3),
        _u("tiled kernel DOWN-sampling by 2.4 (40 -> 17), scalar staging: inputs that no output touches started ABOVE the tile's region "
           "(a negative LDS index before the clamp at 0)", "tiled32", 5, 40, 40, 17, 17, ppb=1, vec=0),
        _u("the same with float4 staging (40 -> 17 x 16)", "tiled32", 5, 40, 40, 17, 16, ppb=1, vec=1),
    ]


def pool_args(c):
    """arg-max pixel of every plane for the fused pool gradient, cycling through: pixel 0, the last pixel, the first tile's last row and
    column, the first pixel of the second tile (the next tile to the right, else below, else pixel 1 of a one-pixel-wider walk), random"""
    Hi, Wi, BC = c["Hi"], c["Wi"], c["BC"]
    ut = 32 if (Hi > 16 or Wi > 16) else 16
    second = ut if Wi > ut else (ut * Wi if Hi > ut else min(1, Hi * Wi - 1))
    special = [0, Hi * Wi - 1, (min(ut, Hi) - 1) * Wi + min(ut, Wi) - 1, second]
    rnd = np.random.default_rng(case_seed(c) + 5).integers(0, Hi * Wi, BC)
    return np.array([special[b % 5] if b % 5 < 4 else rnd[b] for b in range(BC)], np.int32)


# ---------------------------------------------------------------- the tiled backward's per-block tables, emulated
def bwd_axis_tables(n_in, n_out, ut, rm, t):
    """st, wgt, org, ext of tile t of one axis, as the first 2 * UT threads of upsample_bwd_kernel build them"""
    sc = ac_scale(n_in, n_out)
    st = np.zeros(ut, np.int64)
    wgt = np.zeros((ut, UK), F32)
    for li in range(ut):
        i = t * ut + li
        lo = max(0, int(np.floor(F32(i - 1) / sc)) - 1)
        first = -1
        if i < n_in:
            os_ = np.arange(lo, min(n_out, lo + 4 + UK))
            i0, i1, l1 = ac_coord(os_, sc, n_in)
            for o, a, b, l in zip(os_, i0, i1, l1):
                wv = (F32(1) - l if a == i else F32(0)) + (l if b == i else F32(0))
                if first < 0 and (a == i or b == i):
                    first = int(o)
                if first >= 0 and o - first < UK:
                    wgt[li, o - first] = wv
        st[li] = first if first >= 0 else min(lo, n_out - 1)
    org = int(st[0])
    ext = min(min(int(st.max()) + UK - 1, n_out - 1) - org + 1, rm)
    return st, wgt, org, ext


def bwd_axis_effective(n_in, n_out, ut, rm, clamp0=True):
    """(W, bad): W[i, o] the weight the row / column pass gives dy index o for input index i (float64 sums of the fp32 table entries at
    the region index the kernel reads); bad: [(i, k, index)] of reads below 0 or at / beyond ext for an input index inside the map.
    clamp0=False is the index rule before the fix: min(r0 + k, ext - 1) alone."""
    W = np.zeros((n_in, n_out))
    bad = []
    for t in range(cdiv(n_in, ut)):
        st, wgt, org, ext = bwd_axis_tables(n_in, n_out, ut, rm, t)
        for li in range(ut):
            i = t * ut + li
            if i >= n_in:
                continue
            for k in range(UK):
                idx = min(int(st[li]) - org + k, ext - 1)
                if clamp0:
                    idx = max(idx, 0)
                if idx < 0 or idx >= ext:
                    bad.append((i, k, idx))
                else:
                    W[i, org + idx] += np.float64(wgt[li, k])
    return W, bad


# ---------------------------------------------------------------- float64 references of the resize
def axis_matrix(n_in, n_out):
    """dense (n_out, n_in) 1-D interpolation matrix from the forward's own coordinates: weights 1 - l1 and l1, each an fp32 number, held
    as float64"""
    i0, i1, l1 = ac_coord(np.arange(n_out), ac_scale(n_in, n_out), n_in)
    A = np.zeros((n_out, n_in))
    np.add.at(A, (np.arange(n_out), i0), (F32(1) - l1).astype(np.float64))
    np.add.at(A, (np.arange(n_out), i1), l1.astype(np.float64))
    return A


def resize_matrices(Hi, Ho, Wi, Wo):
    return axis_matrix(Hi, Ho), axis_matrix(Wi, Wo)


def coord_delta(n_in):
    """bound of |fp32 source coordinate - exact one|, weights' own rounding included: one rounding of the scale times the largest index
    plus one of the product, 2u (in - 1).  (src >= 1/2: l1 is a multiple of ulp(src) >= 2^-24 and 1 - l1 is exact; src < 1/2: the
    coordinate's error is below 2u src <= u and the rounding of 1 - l1 below u / 2.  The fused l1 drops the product's rounding.)"""
    return 2 * U * (n_in - 1)


def support_matrix(n_in, n_out):
    """S[o, i] = 1 where input i can carry weight for output o under the exact OR the fp32 coordinate (|exact coordinate - i| < 1 + delta)"""
    src = np.arange(n_out) * (float(n_in - 1) / float(n_out - 1) if n_out > 1 else 0.0)
    return (np.abs(src[:, None] - np.arange(n_in)[None, :]) < 1 + coord_delta(n_in)).astype(np.float64)


def _normal(seed, shape):
    return np.random.default_rng(seed).normal(0, 1, shape).astype(np.float32)


@functools.lru_cache(maxsize=2)
def _up_fwd_refs(cid):
    c = UP_FWD_BY_ID[cid]
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    x = _normal(case_seed(c), (BC, Hi, Wi))
    x64 = x.astype(np.float64)
    Ah, Aw = resize_matrices(Hi, Ho, Wi, Wo)
    model = Ah @ x64 @ Aw.T
    bar_model = 8 * U * (np.abs(Ah) @ np.abs(x64) @ np.abs(Aw).T)
    ref = F.interpolate(torch.from_numpy(x64)[None], size=(Ho, Wo), mode="bilinear", align_corners=True)[0].numpy()
    slope_h = np.abs(np.diff(x64, axis=1)).max() if Hi > 1 else 0.0
    slope_w = np.abs(np.diff(x64, axis=2)).max() if Wi > 1 else 0.0
    bar_ref = bar_model + coord_delta(Hi) * slope_h + coord_delta(Wi) * slope_w
    return dict(x=x, model=model, bar_model=bar_model, ref=ref, bar_ref=bar_ref)


def up_fwd_refs(c):
    """x (fp32) and, in float64: model = A_h x A_w^T with bar 8u (|A_h| |x| |A_w|^T) (five roundings on the blend's chain, room for
    contraction); ref = F.interpolate with bar_model + delta_h max|x[h+1] - x[h]| + delta_w max|x[w+1] - x[w]| (the interpolant is
    continuous and piecewise linear: a coordinate error moves it by at most the slope times the error, even where i0 flips)"""
    return _up_fwd_refs(case_id(c))


@functools.lru_cache(maxsize=2)
def _up_bwd_refs(cid):
    c = UP_BWD_BY_ID[cid]
    BC, Hi, Wi, Ho, Wo = c["BC"], c["Hi"], c["Wi"], c["Ho"], c["Wo"]
    seed = case_seed(c)
    dy = _normal(seed + 1, (BC, Ho, Wo))
    pool_g = _normal(seed + 2, (BC,))
    arg = pool_args(c)
    dy64, ady = dy.astype(np.float64), np.abs(dy.astype(np.float64))
    Ah, Aw = resize_matrices(Hi, Ho, Wi, Wo)
    model = Ah.T @ dy64 @ Aw
    scale = np.abs(Ah).T @ ady @ np.abs(Aw)
    kh, kw = int((Ah != 0).sum(0).max()), int((Aw != 0).sum(0).max())
    k = (2 * (kh + kw) + 2) * U
    x0 = torch.zeros(1, BC, Hi, Wi, dtype=torch.float64, requires_grad=True)
    F.interpolate(x0, size=(Ho, Wo), mode="bilinear", align_corners=True).backward(torch.from_numpy(dy64)[None])
    ref = x0.grad[0].numpy()
    Sh, Sw = support_matrix(Hi, Ho), support_matrix(Wi, Wo)
    dh, dw = coord_delta(Hi), coord_delta(Wi)
    coord = dh * (Sh.T @ ady @ np.abs(Aw)) + dw * ((np.abs(Ah) + dh * Sh).T @ ady @ Sw)
    pool = np.zeros((BC, Hi * Wi))
    pool[np.arange(BC), arg] = pool_g.astype(np.float64)
    pool = pool.reshape(BC, Hi, Wi)
    return dict(dy=dy, pool_g=pool_g, pool_arg=arg, model=model, bar_model=k * scale, ref=ref, bar_ref=k * scale + coord,
                model_pool=model + pool, bar_model_pool=k * (scale + np.abs(pool)), kh=kh, kw=kw)


def up_bwd_refs(c):
    """dy, pool_g (fp32), pool_arg and, in float64: model = A_h^T dy A_w with bar (2 (k_h + k_w) + 2) u (|A_h|^T |dy| |A_w|), k the
    largest number of non-zeros in a column of A; model_pool / bar_model_pool with the pool gradient at its arg-max; ref = the autograd
    of F.interpolate with bar_model + the coordinate term: a weight is a hat function of the coordinate, 1-Lipschitz, so it moves by at
    most delta where the support matrix S is set: delta_h S_h^T |dy| |A_w| + delta_w (|A_h| + delta_h S_h)^T |dy| S_w"""
    return _up_bwd_refs(case_id(c))


# ---------------------------------------------------------------- global max-pool
def gmax_fwd_path(HW):
    """global_maxpool_fwd_kernel: float4 scan (8 float4s in flight per thread, a g0 trip covers 8192 elements) when HW % 4 == 0"""
    return ("vector", cdiv(HW // 4, 256 * 8)) if (HW & 3) == 0 else ("scalar", cdiv(HW, 256))


def gmax_owner(i, HW):
    """thread of the block that scans element i"""
    return (i // 4) % 256 if (HW & 3) == 0 else i % 256


def _g(why, kind, BC, HW):
    return dict(why=why, kind=kind, BC=BC, HW=HW, path=gmax_fwd_path(HW)[0], trips=gmax_fwd_path(HW)[1])


GMAX_SIZES = [(1, "a one-pixel plane"), (64, "float4 scan, 16 live threads of one wave"), (1320, "float4 scan, 330 float4s: threads 0..73 scan two"),
              (1323, "scalar scan, six trips (HW % 4 != 0)"), (16384, "float4 scan, the SECOND trip of the g0 loop (the 128 x 128 level)")]
GMAX_FWD = ([_g(w + ", continuous data", "cont", 5, hw) for hw, w in GMAX_SIZES]
            + [_g(w + ", values from {0, 1, 2}: the FIRST of many maxima wins", "ties", 6, hw) for hw, w in GMAX_SIZES]
            + [_g(w + ": an all -inf plane (index 0), planes whose only maximum is the last element", "edges", 4, hw) for hw, w in GMAX_SIZES[1:]])
GMAX_BWD_BIG = dict(why="rsis_global_maxpool_bwd with more than 2^20 elements: the second trip of its grid-stride loop", BC=65, HW=16384)
GMAX_BWD_ADD = dict(why="rsis_global_maxpool_bwd_add into a pre-filled gradient, BC not a multiple of 256: a partial last block", BC=300, HW=64)


def gmax_data(c):
    """x (BC, HW) fp32.  ties: values from {0, 1, 2}; in plane j every 2 before position p_j (0, HW / 3, 7 HW / 8 in turn) is lowered
    to 1, so the first maximum sits in a different thread's share from plane to plane.  edges: plane 0 all -inf; plane 1 continuous
    with the last element raised above everything; plane 2 all -inf but the last element; plane 3 ties {0, 1} with one 2 at the end."""
    BC, HW = c["BC"], c["HW"]
    rs = np.random.default_rng(case_seed(c))
    if c["kind"] == "cont":
        return rs.normal(0, 1, (BC, HW)).astype(np.float32)
    if c["kind"] == "ties":
        x = rs.integers(0, 3, (BC, HW)).astype(np.float32)
        for j in range(BC):
            p = (0, HW // 3, HW - max(1, HW // 8))[j % 3] if HW > 1 else 0
            x[j, :p] = np.minimum(x[j, :p], 1)
        return x
    x = rs.normal(0, 1, (BC, HW)).astype(np.float32)
    x[0] = -np.inf
    x[1, -1] = np.abs(x[1]).max() + 1
    x[2] = -np.inf
    x[2, -1] = -3.0
    x[3] = rs.integers(0, 2, HW)
    x[3, -1] = 2
    return x


def gmax_ref(x):
    """(value, arg) of every plane from F.max_pool2d on a float64 copy"""
    BC, HW = x.shape
    v, i = F.max_pool2d(torch.from_numpy(x).double().view(1, BC, 1, HW), (1, HW), return_indices=True)
    return v.view(BC).numpy(), i.view(BC).numpy()


# ---------------------------------------------------------------- maxpool3x3s2
def maxpool_bwd_path(H, W):
    return "v8" if (H & 1) == 0 and (W & 3) == 0 else "scalar"


def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def _m(why, BC, H, W):
    path = maxpool_bwd_path(H, W)
    return dict(why=why, BC=BC, H=H, W=W, path=path, items=BC * H * W // (8 if path == "v8" else 1))


MAXPOOL = [
    _m("v8, one 2 x 4 block per row pair", 8, 8, 8), _m("scalar, odd sizes", 15, 9, 11), _m("scalar, H even but W % 4 != 0", 2, 16, 6),
    _m("scalar, odd square", 6, 7, 7), _m("v8, several blocks per row", 6, 12, 20), _m("v8, one block per row (W = 4)", 2, 10, 4),
    _m("v8, the wider map", 16, 32, 64), _m("scalar, a one-row map", 6, 1, 9), _m("scalar, a one-column map", 6, 9, 1), _m("scalar, a one-pixel map", 2, 1, 1),
    _m("v8, a single 2 x 4 block: every window hangs over an edge", 3, 2, 4),
    _m("scalar backward with more than 2^20 pixels: the second trip of its grid-stride loop", 259, 63, 65),
    _m("v8 backward with more than 2^20 blocks of 8 pixels (the smallest map that reaches its second trip is 32 MiB) and a forward with "
       "more than 2^20 outputs", 2049, 64, 64),
]


def maxpool_data(c, ties):
    """x fp32 (clamped to [-0.5, 0.5] for ties: most windows hold several 0.5s and the FIRST takes the gradient), integer dy and prefill, |.| <= 3:
    sums of up to four such terms and the prefill are exact in fp32"""
    BC, H, W = c["BC"], c["H"], c["W"]
    rs = np.random.default_rng(case_seed(c))
    x = rs.normal(0, 1, (BC, H, W)).astype(np.float32)
    if ties:
        x = np.clip(x, np.float32(-0.5), np.float32(0.5))
    dy = rs.integers(-3, 4, (BC, pool_out(H), pool_out(W))).astype(np.float32)
    pre = rs.integers(-3, 4, (BC, H, W)).astype(np.float32)
    return x, dy, pre


def maxpool_ref(x, dy):
    """(value, flat arg-max index in the plane, gradient) from F.max_pool2d on a float64 copy"""
    BC, H, W = x.shape
    v, i = F.max_pool2d(torch.from_numpy(x).double()[None], 3, 2, 1, return_indices=True)
    g = torch.zeros(BC, H * W, dtype=torch.float64)
    g.scatter_add_(1, i[0].reshape(BC, -1), torch.from_numpy(dy).double().reshape(BC, -1))
    return v[0].numpy(), i[0].numpy(), g.view(BC, H, W).numpy()


UP_FWD = _up_fwd_cases()
UP_BWD = _up_bwd_cases()
UP_FWD_BY_ID = {case_id(c): c for c in UP_FWD}
UP_BWD_BY_ID = {case_id(c): c for c in UP_BWD}
assert len(UP_FWD_BY_ID) == len(UP_FWD) and len(UP_BWD_BY_ID) == len(UP_BWD)
