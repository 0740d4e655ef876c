"""Case tables of the training-call conv tests (test_gpu_train_paths.py on the GPU, test_train_paths_host.py on the host): plain data, the
dispatch rules of the library restated as small pure functions, and the float64 references.  Nothing here touches the GPU.

A conv case is a dict: B, segs (channel counts of the concat sources -- for a data gradient: of the destinations), H, W (the conv's INPUT
map), cout, ks, stride, pad, and flags bias / addend.  Every case carries a `why`: the edge it is the smallest instance of."""
import numpy as np
import torch
import torch.nn.functional as F

CK = 8                          # RSIS_CK: channels per chunk of conv3x3_direct.hip
FLUSH_MIN_CHUNKS = 48           # RSIS_FLUSH_MIN_CHUNKS: a slice this long runs the segmented instantiation
EXACT_LIMIT = 2 ** 24

# variant code -> (rows BM, tile width TW, tile height TH) of launch_direct_epi() in conv3x3_direct.hip
DIRECT_GEOM = {1: (64, 8, 8), 2: (64, 16, 8), 3: (64, 32, 8), 4: (32, 16, 8), 5: (32, 32, 8), 6: (32, 8, 8), 7: (64, 32, 16), 8: (32, 32, 16),
               9: (64, 16, 16)}
DIRECT_TILES = list(range(10))                      # 0: the dispatcher's own choice
S2_DGRAD_TILES = [0, 1, 2, 3, 4, 5, 6]              # EPI_S2: 1, 2, 4, 5 exist, 3 runs 5, 6 runs 1 (7-9 are refused)
F2_TILES = [0, 1, 4]                                # EPI_F2: 1 and 4 exist, everything else is the dispatcher's choice
IGEMM_TILES = [0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16]     # launch_ks() of conv_igemm.hip; 0 = its own choice (one of 11-16)


def _c(why, B, segs, H, W, cout, ks=3, stride=1, pad=1, bias=False, addend=False, **kw):
    d = dict(why=why, B=B, segs=list(segs), H=H, W=W, cout=cout, ks=ks, stride=stride, pad=pad, bias=bias, addend=addend)
    d.update(kw)
    return d


def _base_id(c):
    return "%s%dx%ds%d_B%d_%s_%dx%d_co%d%s%s" % (c.get("tag", ""), c["ks"], c["ks"], c["stride"], c["B"], "+".join(map(str, c["segs"])), c["H"], c["W"],
                                               c["cout"], "_b" if c["bias"] else "", "_a" if c["addend"] else "")


def case_id(c):
    return _base_id(c) + ("_inplace" if c.get("inplace") else "") + ("_sub" if c.get("subsample") else "")


def case_seed(c):
    """seed of a case's data, from its geometry alone: the in-place scatter draws the dy and weights of the fresh one"""
    return 7000 + 13 * (sum(map(ord, _base_id(c))) % 977)


def cdiv(a, b):
    return (a + b - 1) // b


def chunks(segs):
    return sum(cdiv(c, CK) for c in segs)


def out_size(c):
    return ((c["H"] + 2 * c["pad"] - c["ks"]) // c["stride"] + 1, (c["W"] + 2 * c["pad"] - c["ks"]) // c["stride"] + 1)


# ---------------------------------------------------------------- the split-K rules, restated
def api_allows_split(B, H, W, rows, nq, addend_blocks=False):
    """the gate of api.hip (rsis_conv2d_fwd with tile + 100, rsis_conv2d_dgrad): nq >= 32 chunks and px_tiles * ceil(rows / 64) < 160 with
    px_tiles = B * ceil(H / 8) * ceil(W / (8 if W <= 8 else 16)); a data gradient with an addend is never split (addend_blocks)"""
    px_tiles = B * cdiv(H, 8) * cdiv(W, 8 if W <= 8 else 16)
    return (not addend_blocks) and nq >= 32 and px_tiles * cdiv(rows, 64) < 160


def small_map_variant(B, H, W, rows, split_allowed):
    """pick_direct_variant<EPI_PLAIN>() on maps <= 8 x 8, the only maps the split-K cases use: 1 where the grid split is allowed and
    ceil(rows / 64) * B < 160, else 6 below 1024 such blocks, else 1"""
    assert H <= 8 and W <= 8
    b64 = cdiv(rows, 64) * B
    return 1 if (split_allowed and b64 < 160) or b64 >= 1024 else 6


def direct_ksplit(B, H, W, rows, nq, variant):
    """launch_direct_cfg() once api.hip has allowed the split: blocks = ceil(rows / BM) * ceil(W / TW) * ceil(H / TH) * B; below 160 blocks
    (and from 32 chunks) ksplit = min(ceil(512 / blocks), nq // 8, 16), at least 1"""
    bm, tw, th = DIRECT_GEOM[variant]
    blocks = cdiv(rows, bm) * cdiv(W, tw) * cdiv(H, th) * B
    if blocks >= 160 or nq < 32:
        return 1
    return max(1, min(cdiv(512, blocks), nq // 8, 16))


def slice_chunks(nq, ksplit):
    """chunks per slice: slice kz walks [nq * kz // ksplit, nq * (kz + 1) // ksplit)"""
    return [nq * (kz + 1) // ksplit - nq * kz // ksplit for kz in range(ksplit)]


def split_plan(c, tile, dgrad=False, deterministic=False):
    """(variant, ksplit, chunks per slice, segmented?) of a split-K case; the deterministic mode allows no split (and the dispatcher then
    picks variant 6 on these maps).  For a data gradient the reduction runs over the cout rows of dy and the output rows are the
    destination channels."""
    rows, nq = (sum(c["segs"]), cdiv(c["cout"], CK)) if dgrad else (c["cout"], chunks(c["segs"]))
    allowed = (not deterministic) and api_allows_split(c["B"], c["H"], c["W"], rows, nq, addend_blocks=dgrad and c["addend"])
    variant = tile if tile else small_map_variant(c["B"], c["H"], c["W"], rows, allowed)
    ks = direct_ksplit(c["B"], c["H"], c["W"], rows, nq, variant) if allowed else 1
    sl = slice_chunks(nq, ks)
    return variant, ks, sl, (variant <= 6 and nq // ks >= FLUSH_MIN_CHUNKS)


# ---------------------------------------------------------------- 1. exact regime
# direct 3x3 / stride 1; the same shapes run as the forward (segs -> cout) and as the data gradient (dy with cout rows -> segs)
DIRECT_EXACT = [
    _c("9 x 17: one row past the 8-row tiles and one column past the 16-wide ones; 33 channels: the fifth chunk holds one channel; 40 rows: "
       "the tail of a 32- and of a 64-row block; bias + addend in one epilogue / a single-destination gradient", 2, [33], 9, 17, 40, bias=True,
       addend=True),
    _c("17 x 33: one row past the 16-row tiles (variants 7-9), one column past the 32-wide ones; two sources with channel tails (3 + 2 chunks); "
       "72 rows: the tail of the second 64-row block; two destinations", 1, [20, 12], 17, 33, 72, bias=True),
    _c("9 x 9: one pixel past the 8 x 8 tile both ways; three sources (2 + 2 + 1 chunks) / three destinations; addend without a bias", 2, [16, 16, 8],
       9, 9, 40, addend=True),
]
DIRECT_DGRAD_EXACT = [dict(c, bias=False, addend=False) for c in DIRECT_EXACT] + [
    dict(DIRECT_EXACT[0], bias=False, addend=True, why="a single-destination gradient with the gradient hand-over addend (fast epilogue)")]

# grid split-K (default mode; the deterministic mode runs them unsplit).  `slices`: what the comment claims, asserted on the host against
# split_plan() for variant 1, the variant the dispatcher picks for every one of them.
SPLIT_FWD = [
    _c("33 chunks in four slices of 8 / 8 / 8 / 9, the last chunk holds one channel; two blocks", 2, [257], 8, 8, 40, slices=[8, 8, 8, 9], seg=False,
       tiles=DIRECT_TILES),
    _c("256 chunks in 16 slices (the cap) of 16; 4 x 4 map: most of every tile is outside the image", 2, [2048], 4, 4, 64, slices=[16] * 16, seg=False,
       tiles=[0, 1, 2, 4, 6, 9]),
    _c("192 chunks in four slices of 48 = RSIS_FLUSH_MIN_CHUNKS: the segmented instantiation with the grid split on top; 128 blocks of 64 rows "
       "(the 32-row variants make 256 blocks, are not split and run segmented over all 192 chunks)", 128, [1536], 4, 4, 64, slices=[48] * 4,
       seg=True, tiles=[0, 1, 2, 4, 9]),
]
SPLIT_FWD = [dict(c, bias=b, tag="split_") for c in SPLIT_FWD for b in (False, True)]
SPLIT_DGRAD = [
    _c("data gradient of a gate conv with 256 rows (32 chunks, four slices of 8) on an 8 x 8 map into two destinations: every destination "
       "zeroed, atomics into both", 2, [24, 16], 8, 8, 256, slices=[8] * 4, seg=False, tiles=DIRECT_TILES, tag="split_"),
]

# 3x3 / stride 2 / pad 1: forward (EPI_F2) and data gradient (EPI_S2); H x W is the conv's input map = the gradient's dx map
_S2_MAPS = [
    (17, 15, "odd x odd: the last parity row and column of dx exist only in class (0, 0); two tile rows"),
    (9, 64, "odd x even, wide: 32 dy columns = one 32-wide tile exactly / two 16-wide tiles, the odd last dx row"),
    (1, 12, "a 1-pixel-high map: one dy row, the classes with ph = 1 write nothing"),
    (16, 7, "even x odd: the last dx column has no odd neighbour"),
    (8, 12, "even x even: every class writes a full quarter"),
]
S2_EXACT = [_c(why, 2, [20], H, W, 40, stride=2, bias=True) for H, W, why in _S2_MAPS]

# implicit GEMM (conv_igemm.hip), forward calls
IGEMM_FWD_EXACT = [
    _c("1x1 on the LDS-DMA path: H W = 36 and 160 channels (5 K-tiles of 32, 10 of 16); 72 pixels: a partial pixel tile at every tile width; "
       "40 rows: row tail", 2, [160], 6, 6, 40, ks=1, pad=0, bias=True, nst=True),
    _c("1x1 off the LDS-DMA path: a 7 x 7 map (49 pixels per image) and 40 channels (a ragged K-tile)", 2, [40], 7, 7, 72, ks=1, pad=0, addend=True),
    _c("1x1 / stride 2 as the gather: 9 x 7 -> 5 x 4", 2, [40], 9, 7, 40, ks=1, stride=2, pad=0, bias=True),
    _c("1x1 / stride 2 on the sub-sampled copy (rsis_subsample2d, then the stride-1 GEMM): 10 x 8 -> 5 x 4 = 20 pixels, 64 channels: LDS-DMA",
       2, [64], 10, 8, 40, ks=1, stride=2, pad=0, bias=True, subsample=True),
    _c("the 7x7 / stride 2 / pad 3 stem on an odd map (13 x 11 -> 7 x 6): 49 taps, the 64-bit tap mask, K = 147 (ragged K-tile)", 2, [3], 13, 11, 40,
       ks=7, stride=2, pad=3, bias=True),
]
# ... and data gradients: segs are the destinations, cout the rows of dy, H x W the dx map
IGEMM_DGRAD_EXACT = [
    _c("1x1 / stride 1 gradient = a 1x1 conv over dy: 96 rows (3 K-tiles of 32: fewer than a ring of depth 4 holds) on the LDS-DMA path", 2, [40], 6, 6,
       96, ks=1, pad=0, nst=True),
    _c("1x1 / stride 1 gradient with the hand-over addend, off the LDS-DMA path", 2, [24], 7, 7, 40, ks=1, pad=0, addend=True),
    _c("1x1 / stride 2 scatter into a zeroed dx: only the even pixels of a 9 x 7 map receive a gradient", 2, [24], 9, 7, 40, ks=1, stride=2, pad=0),
    _c("1x1 / stride 2 scatter IN PLACE into a prefilled dx (addend == dx[0]): the prefill survives at the odd pixels, is added once at the even "
       "ones", 2, [24], 9, 7, 40, ks=1, stride=2, pad=0, inplace=True),
    _c("the stem's DGRAD gather: 7x7 / stride 2 / pad 3, parity of every tap", 2, [3], 13, 11, 40, ks=7, stride=2, pad=3),
    _c("launch_ks<3, true>: a 3x3 / stride 2 gradient into TWO destinations (the parity-class kernel writes one)", 2, [12, 8], 9, 7, 40, stride=2),
]

# conv_c1.hip at one step (cout = 1); `c1`: whether the vector kernel takes the call (else the MFMA path through the same entry points)
C1_EXACT = [
    _c("8 channels, 64-wide tile, partial tile rows", 2, [8], 12, 64, 1, bias=True, c1=True),
    _c("16 channels (several channel passes), the 128-wide tile on a 72-wide image", 2, [16], 20, 72, 1, bias=True, c1=True),
    _c("4 channels, the 256-wide tile on a 160-wide image, a partial second tile row", 2, [4], 9, 160, 1, bias=True, c1=True),
    _c("the neighbour with 6 channels: rsis_c1_supported() is false, the direct MFMA kernel with one output row", 2, [6], 12, 64, 1, bias=True, c1=False),
    _c("the neighbour with W % 4 != 0", 2, [8], 12, 66, 1, bias=True, c1=False),
]

# ---------------------------------------------------------------- 2. normal regime (reduced)
DIRECT_NORMAL = [
    _c("channel tails over two sources, partial tiles both ways, row tail", 2, [20, 12], 9, 17, 40, bias=True),
    _c("9 chunks, 17 x 33, 72 rows", 1, [72], 17, 33, 72),
]
SPLIT_NORMAL = [dict(c, tiles=[0, 1, 4] if c["segs"] != [257] else [0, 1, 4, 6, 9]) for c in SPLIT_FWD if c["bias"]]
SPLIT_DGRAD_NORMAL = [dict(SPLIT_DGRAD[0], tiles=[0, 1, 4])]
S2_NORMAL = [S2_EXACT[0], S2_EXACT[1]]
IGEMM_FWD_NORMAL = [IGEMM_FWD_EXACT[0], IGEMM_FWD_EXACT[1], IGEMM_FWD_EXACT[2], IGEMM_FWD_EXACT[4]]
IGEMM_DGRAD_NORMAL = [IGEMM_DGRAD_EXACT[0], IGEMM_DGRAD_EXACT[3], IGEMM_DGRAD_EXACT[4], IGEMM_DGRAD_EXACT[5]]
TIGHT_IMAGES = 16               # the host models of the 128-image case cover its first 16 images (the tight bar is taken over those)

# ---------------------------------------------------------------- 3. ConvLSTM: LSTM_CASES of test_gpu_infer_paths.py
LSTM_CASES = [
    # (B, [x segs], hid, H, W)
    (2, [8], 4, 5, 7),
    (2, [16, 16], 8, 16, 16),
    (2, [6, 5], 3, 6, 5),
    (2, [64, 64], 32, 8, 8),
    (1, [128], 128, 4, 4),
    (2, [24], 16, 9, 12),
]


# ---------------------------------------------------------------- data and float64 references
def ints(seed, shape, nonzero=False):
    v = np.random.default_rng(seed).integers(-3, 4, shape)
    if nonzero:
        v = np.where(v == 0, 3, v)
    return v.astype(np.float32)


def normal(seed, shape, scale=1.0):
    return np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32)


def exact_bound(c, dgrad=False):
    """an upper bound on sum |terms| of any output of the exact regime: every operand is an integer with |v| <= 3, so a product is at
    most 9 and there are at most K of them, plus bias, addend / prefill"""
    K = (c["cout"] if dgrad else sum(c["segs"])) * c["ks"] ** 2
    return 9 * K + 3 + 3


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def fwd_data(c, regime, seed):
    """inputs of a forward call and its float64 reference: dict xs (list), w, b, add (or None), ref (float64 tensor)"""
    gen = ints if regime == "exact" else normal
    C = sum(c["segs"])
    Ho, Wo = out_size(c)
    xs = [gen(seed + i, (c["B"], s, c["H"], c["W"])) for i, s in enumerate(c["segs"])]
    w = ints(seed + 5, (c["cout"], C, c["ks"], c["ks"]), nonzero=True) if regime == "exact" else \
        normal(seed + 5, (c["cout"], C, c["ks"], c["ks"]), 1.0 / np.sqrt(C * c["ks"] ** 2))
    b = gen(seed + 6, (c["cout"],)) if c["bias"] else None
    add = gen(seed + 7, (c["B"], c["cout"], Ho, Wo)) if c["addend"] else None
    ref = F.conv2d(torch.cat([_t(x) for x in xs], 1).double(), _t(w).double(), _t(b).double() if b is not None else None, stride=c["stride"],
                   padding=c["pad"])
    if add is not None:
        ref = ref + _t(add).double()
    return dict(xs=xs, w=w, b=b, add=add, ref=ref)


def dgrad_data(c, regime, seed):
    """inputs of a data-gradient call and its float64 references: dy (B, cout, Hy, Wy), w (cout, sum segs, ks, ks), add (the addend, or the
    prefill of an in-place call; None), refs: one float64 tensor per destination"""
    gen = ints if regime == "exact" else normal
    C = sum(c["segs"])
    Hy, Wy = out_size(c)
    dy = gen(seed, (c["B"], c["cout"], Hy, Wy))
    w = ints(seed + 5, (c["cout"], C, c["ks"], c["ks"]), nonzero=True) if regime == "exact" else \
        normal(seed + 5, (c["cout"], C, c["ks"], c["ks"]), 1.0 / np.sqrt(c["cout"] * c["ks"] ** 2))
    add = gen(seed + 7, (c["B"], C, c["H"], c["W"])) if (c["addend"] or c.get("inplace")) else None
    if add is not None and regime == "exact":
        add = np.where(add == 0, np.float32(2), add)            # a prefill that is lost or added twice shows at every pixel
    oph, opw = c["H"] - ((Hy - 1) * c["stride"] - 2 * c["pad"] + c["ks"]), c["W"] - ((Wy - 1) * c["stride"] - 2 * c["pad"] + c["ks"])
    ref = F.conv_transpose2d(_t(dy).double(), _t(w).double(), stride=c["stride"], padding=c["pad"], output_padding=(oph, opw))
    assert tuple(ref.shape) == (c["B"], C, c["H"], c["W"])
    if add is not None:
        ref = ref + _t(add).double()
    return dict(dy=dy, w=w, add=add, refs=list(ref.split(c["segs"], 1)))
