"""Case tables, input builders, float64 references and host models of test_gpu_loss_path.py (and of test_loss_path_host.py, which checks
them without a device): the soft-IoU sums and backward (csrc/losses.hip), the class / stop heads, the loss tail, and the two assignment
kernels of csrc/pointwise.hip.  Everything here is numpy on the host; nothing imports the library.

  float64 reference : the operation on the SAME fp32 inputs, every intermediate in float64;
  host model        : the operation in numpy float32, every sum ONE sequential fp32 chain (np.cumsum of float32 is such a chain); its
                      distance from the float64 reference, err_host, is the yardstick of a normal-regime bar (m * err_host);
  exact regime      : inputs chosen so that every fp32 operation of the kernel is exact in any order -- the result must EQUAL float64."""
import numpy as np

U24 = 2.0 ** -24                      # one fp32 rounding, relative
F32 = np.float32


def _rng(seed):
    return np.random.default_rng(seed)


def sigmoid32(x):
    """rsis_sigmoid (common.h) in numpy float32: 1 / (1 + exp(-x)), each operation rounded to fp32"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x, dtype=F32))).astype(F32)


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def chain32(a, axis=-1):
    """sum of a float32 array along `axis` as one sequential fp32 chain, first element first"""
    a = np.asarray(a, F32)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), F32)
    return np.take(np.cumsum(a, axis=axis, dtype=F32), -1, axis=axis)


# ======================================================================================================================
# 1. soft-IoU
# ======================================================================================================================
EXACT_LOGITS = (-100.0, 0.0, 30.0)    # fp32 sigmoid: 1 / (1 + inf) = 0,  1 / 2,  1 / (1 + 9.4e-14) = 1


def _iou(B, T, G, N, why, **expect):
    return dict(B=B, T=T, G=G, N=N, why=why, expect=expect)


# (B, T, G, N): the smallest shapes that cross each rule of rsis_l_softiou_sums (restated in sums_plan below; `expect` holds the
# fields of the default-mode plan the comment claims -- test_loss_path_host.py compares)
IOU_ONES = [
    _iou(2, 1, 1, 8, "the smallest call: one wave per image, one 8-pixel tail step", kernel="ones", per=64, waves=1, last=8),
    _iou(1, 31, 31, 520, "the widest ones-row tile (row / column 31 = the ones); 8 full waves and a ninth with 8 pixels", kernel="ones", per=64, waves=9, last=8),
    _iou(3, 10, 20, 4096, "the training shape at 64 x 64, three images", kernel="ones", per=64, waves=64, last=64),
    _iou(2, 31, 5, 72, "T at the limit, few GT slots; second wave holds 8 pixels", kernel="ones", per=64, waves=2, last=8),
    _iou(2, 5, 31, 72, "G at the limit, few predictions", kernel="ones", per=64, waves=2, last=8),
    _iou(32, 10, 20, 392 * 4 * 2 + 8, "the bench batch: 32 splits are offered, per_wave falls to its floor of 64, the 50th wave holds 8 pixels",
         kernel="ones", per=64, waves=50, last=8),
    _iou(32, 2, 3, 127 * 392 + 8, "per_wave 392 = 12 * 32 + 8, the value of the 224 x 224 bench batch (N = 50176, 32 images): twelve trips of the "
         "main loop and one tail step in every wave, all 128 waves of an image busy, the last one with 8 pixels", kernel="ones", per=392, waves=128, last=8),
    _iou(1, 3, 4, 524288, "the 512 x 1024 map: per_wave 128, 4096 waves; deterministic mode: one lane chain of 262144 terms", kernel="ones", per=128, waves=4096, last=128),
]
IOU_TILED = [
    _iou(2, 32, 1, 64, "T = 32 opens the tiled kernel with one G slot", kernel="tiled", nT=1, nG=1, tshift=0, groups=4, per=64, pgroups=1),
    _iou(2, 1, 32, 64, "G = 32 opens it with one prediction", kernel="tiled", nT=1, nG=1, tshift=0, groups=4, per=64, pgroups=1),
    _iou(1, 33, 33, 520, "one row past a tile in both directions: nT = nG = 2, two waves per pixel group", kernel="tiled", nT=2, nG=2, tshift=1, groups=2, per=64, pgroups=9),
    _iou(2, 64, 64, 264, "two full tiles each way; the fifth pixel group holds 8 pixels", kernel="tiled", nT=2, nG=2, tshift=1, groups=2, per=64, pgroups=5),
    _iou(1, 65, 127, 136, "nT = 3: tshift 2, the wave of T tile 3 returns early; nG = 4 with a ragged last tile", kernel="tiled", nT=3, nG=4, tshift=2, groups=1, per=64, pgroups=3),
    _iou(1, 128, 128, 520, "the largest call: 4 x 4 tiles", kernel="tiled", nT=4, nG=4, tshift=2, groups=1, per=64, pgroups=9),
    _iou(2, 96, 100, 72, "nT = 3 full tiles, nG = 4 ragged", kernel="tiled", nT=3, nG=4, tshift=2, groups=1, per=64, pgroups=2),
]
IOU_CASES = IOU_ONES + IOU_TILED
IOU_BWD_ONLY = [_iou(1, 9, 3, 1048576, "2.36 M float4 against the backward's grid cap of 2.10 M threads: the grid-stride loop takes a second trip")]
IOU_BWD_GRID_CAP = 256 * 32 * 256     # rsis_l_softiou_bwd: at most 256 * 32 blocks of 256 threads
MIN_TERMS = 2 ** 14                   # a normal case is judged by the largest error over its sums: it needs that many summed terms (sums x pixels)
                                      # behind it for that maximum to measure the summation and not the luck of a few roundings
IOU_REGIMES = {"n2": 2.0, "hot": 12.0}     # N(0, 2) as the older tests; N(0, 12): most pixels saturated, as a trained decoder emits


def iou_id(c):
    return "b%d_t%d_g%d_n%d" % (c["B"], c["T"], c["G"], c["N"])


def iou_seed(c):
    return (c["B"] * 7 + c["T"] * 131 + c["G"] * 17 + c["N"]) % 100003


def iou_population(c):
    return c["B"] * (c["T"] * c["G"] + c["T"] + c["G"])


IOU_NORMAL = [c for c in IOU_CASES if iou_population(c) * c["N"] >= MIN_TERMS]


def sums_plan(B, T, G, N, deterministic=False):
    """rsis_l_softiou_sums (losses.hip) restated: which kernel, how many pixels per wave / pixel group, how many of them hold pixels"""
    r8 = lambda v: (v + 7) // 8 * 8
    if T >= 32 or G >= 32:
        nT, nG = (T + 31) // 32, (G + 31) // 32
        tshift = 0 if nT <= 1 else 1 if nT == 2 else 2
        groups = 4 >> tshift
        nblk = (1024 + B - 1) // B
        per = max(64, r8((N + nblk * groups - 1) // (nblk * groups)))
        if deterministic:
            per = r8(N)
        return dict(kernel="tiled", nT=nT, nG=nG, tshift=tshift, groups=groups, per=per, pgroups=(N + per - 1) // per)
    nsplit = (1024 + B - 1) // B
    per = max(64, r8((N + nsplit * 4 - 1) // (nsplit * 4)))
    if deterministic:
        per = r8(N)
    waves = (N + per - 1) // per
    return dict(kernel="ones", per=per, waves=waves, last=N - (waves - 1) * per)


def _iou_masks(rs, B, G, N):
    """GT masks in {0, 1} with one all-zero and one all-one slot per image (G = 1: images alternate)"""
    y = (rs.random((B, G, N)) < 0.3).astype(F32)
    if G >= 2:
        y[:, 0], y[:, -1] = 0, 1
    else:
        y[0::2, 0], y[1::2, 0] = 0, 1
    return y


def _iou_perm(rs, B, T, G):
    """perm (B, perm_ld) int64 with perm_ld = max(T, G) + 3: a permutation of the GT slots over the first min(T, G) predictions, repeated
    slots for t >= G, and VALID but unrelated slots in the padding (a wrong leading dimension then reads wrong masks, never out of range)"""
    ld = max(T, G) + 3
    perm = rs.integers(0, G, (B, ld))
    for b in range(B):
        k = min(T, G)
        perm[b, :k] = rs.permutation(G)[:k]
    return perm.astype(np.int64)


def sums64(p, y):
    """S (B, T+1, G+1) float64 from probabilities p (B, T, N) and masks y (B, G, N), any float dtype: [t][g] intersections,
    [t][G] = sum p, [T][g] = sum y, [T][G] = 0 (what rsis_softiou_sums leaves there)"""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    B, T, _ = p.shape
    G = y.shape[1]
    S = np.zeros((B, T + 1, G + 1))
    S[:, :T, :G] = np.matmul(p, y.transpose(0, 2, 1))
    S[:, :T, G] = p.sum(-1)
    S[:, T, :G] = y.sum(-1)
    return S


def sums_chain32(logits, y):
    """the host model of rsis_softiou_sums: fp32 sigmoid, fp32 products, one sequential fp32 chain over the pixels per sum"""
    p = sigmoid32(logits)
    B, T, N = p.shape
    G = y.shape[1]
    S = np.zeros((B, T + 1, G + 1), F32)
    for b in range(B):
        for t in range(T):
            S[b, t, :G] = chain32(p[b, t][None, :] * y[b])
        S[b, :T, G] = chain32(p[b])
        S[b, T, :G] = chain32(y[b])
    return S


def cost64(S, e=1e-6):
    """all-pairs cost (B, G, T) of train.py:102-110 / hungarian.py:62-89 from the sums: 1 - I / (sum p + sum y - I + e)"""
    inter = S[:, :-1, :-1]
    den = S[:, :-1, -1:] + S[:, -1:, :-1] - inter + e
    return (1 - inter / den).transpose(0, 2, 1), den.transpose(0, 2, 1)


def iou_bwd64(logits, y, perm, ca, cb, p=None):
    """(ca y + cb (1 - y)) p (1 - p) with y = Y[b][perm[b][t]], float64; p: the probabilities where they are not float64's sigmoid
    (the exact regime: the fp32 sigmoid's 0, 1/2, 1)"""
    B, T, _ = logits.shape
    p = sigmoid64(logits) if p is None else np.asarray(p, np.float64)
    yy = np.stack([y[b, perm[b, :T]] for b in range(B)]).astype(np.float64)
    a, c = ca.astype(np.float64)[:, :, None], cb.astype(np.float64)[:, :, None]
    return (a * yy + c * (1 - yy)) * p * (1 - p)


def iou_exact_data(c, with_sums=True):
    """logits from EXACT_LOGITS, masks in {0, 1}; integer ca / cb; the float64 sums (counts in halves) and gradient"""
    B, T, G, N = c["B"], c["T"], c["G"], c["N"]
    rs = _rng(iou_seed(c))
    logits = np.array(EXACT_LOGITS, F32)[rs.integers(0, 3, (B, T, N))]
    y = _iou_masks(rs, B, G, N)
    perm = _iou_perm(rs, B, T, G)
    ca = rs.integers(-3, 4, (B, T)).astype(F32)
    cb = rs.integers(-3, 4, (B, T)).astype(F32)
    d = dict(logits=logits, y=y, perm=perm, ca=ca, cb=cb)
    if with_sums:
        d["S"] = sums64(sigmoid32(logits), y)
    d["dlogits"] = iou_bwd64(logits, y, perm, ca, cb, sigmoid32(logits))
    return d


# dlogits = (a y + c (1 - y)) * p * (1 - p), y in {0, 1}: the coefficient is a or c EXACTLY.  Roundings, in units of 2^-24:
#   p = 1 / (1 + expf(-x)): expf 2 (its error reaches p scaled by e / (1 + e) <= 1), the addition 1, the division 1        -> 4, relative to p
#   1 - p: one rounding, relative; and the ABSOLUTE error 4 u p of p, which is not small against 1 - p when p is near 1          -> 1
#   the two products                                                                                                             -> 2
# so |err| <= 7 u |ref| + |coef| p * 4 u p <= 7 u |ref| + 7 u max|coef|.
K_DLOGITS = 7


def iou_normal_data(c, regime):
    """seeded N(0, scale) logits; float64 references and the host model's error, the largest over the case"""
    B, T, G, N = c["B"], c["T"], c["G"], c["N"]
    rs = _rng(iou_seed(c) + (1 if regime == "hot" else 0))
    logits = rs.normal(0, IOU_REGIMES[regime], (B, T, N)).astype(F32)
    y = _iou_masks(rs, B, G, N)
    perm = _iou_perm(rs, B, T, G)
    S = sums64(sigmoid64(logits), y)
    err_host = float(np.abs(sums_chain32(logits, y).astype(np.float64) - S).max())
    cost, den = cost64(S)
    ca = rs.normal(0, 1, (B, T)).astype(F32) / F32(N)            # the size of -g / U
    cb = rs.normal(0, 1, (B, T)).astype(F32) / F32(N)
    return dict(logits=logits, y=y, perm=perm, S=S, err_host=err_host, cost=cost, den=den, ca=ca, cb=cb,
                dlogits=iou_bwd64(logits, y, perm, ca, cb))


# ======================================================================================================================
# 2. heads
# ======================================================================================================================
HEADS_MAXK, HEADS_MAXC, LDS_FLOATS = 2048, 64, 64 * 1024 // 4
HEADS_SHAPES = [(2, [1], 1), (3, [5], 2), (320, [128, 64, 32, 16, 8], 21), (97, [16, 8], 33), (64, [2048], 64), (7, [100, 3, 9, 1, 50], 17)]
# the exact backward hands in probs = 1 / npow, npow the power of two >= ncls (so 1 / ncls for 1, 2, 64); two more shapes bring ncls 4 and 16
HEADS_BWD_EXACT = HEADS_SHAPES + [(5, [24, 8], 4), (33, [40], 16)]
HEADS_NORMAL = [s for s in HEADS_SHAPES if s[0] * s[2] >= 100]     # enough outputs for a max of errors to mean something (and ncls > 1)
HEADS_LIMIT = ([128, 64, 32, 16, 8], 21)                           # the decoder's heads at hidden 128: K = 248


def heads_id(s):
    return "r%d_k%s_c%d" % (s[0], "+".join(str(c) for c in s[1]), s[2])


def heads_seed(s):
    return (s[0] * 31 + sum(s[1]) * 7 + s[2]) % 100003


def heads_lds_floats(rows, K, ncls):
    """rsis_l_heads_bwd: 2 rows (ncls + 1) + rows ceil(K / rows) floats of dynamic LDS"""
    return 2 * rows * (ncls + 1) + rows * ((K + rows - 1) // rows)


def heads_fits(rows, K, ncls):
    return 1 <= K <= HEADS_MAXK and 1 <= ncls <= HEADS_MAXC and rows >= 1 and heads_lds_floats(rows, K, ncls) <= LDS_FLOATS


def heads_max_rows(K, ncls):
    """(the largest row count rsis_heads_bwd accepts, the first it refuses) -- above K the rule is monotone: rows (2 ncls + 3) floats"""
    rows = K
    while heads_fits(rows + 1, K, ncls):
        rows += 1
    return rows, rows + 1


def _ints(rs, shape, nonzero=False):
    a = rs.integers(-3, 4, shape)
    if nonzero:
        a = np.where(a == 0, 2, a)
    return a.astype(F32)


def heads_bwd64(sides, Wc, Ws, probs, dprobs, dstop):
    """softmax backward dl = p (g - sum g p), d stop; d side = dl Wc + dstop Ws; the parameter gradients summed over the rows.  float64.
    dprobs / dstop None = zero (a null pointer)."""
    sv = np.concatenate(sides, 1).astype(np.float64)
    p = probs.astype(np.float64)
    g = dprobs.astype(np.float64) if dprobs is not None else np.zeros_like(p)
    ds = dstop.astype(np.float64) if dstop is not None else np.zeros(p.shape[0])
    dl = p * (g - (g * p).sum(1, keepdims=True))
    dside = dl @ Wc.astype(np.float64) + ds[:, None] * Ws.astype(np.float64)[None, :]
    return dict(dside=dside, dWc=dl.T @ sv, dbc=dl.sum(0), dWs=ds @ sv, dbs=np.array([ds.sum()]), dl=dl)


def heads_exact_data(s):
    """integers in -3..3 everywhere; probs 1 / npow.  The stop logit, every d-logit (dyadic) and every sum are exact in fp32."""
    rows, Cs, ncls = s
    rs = _rng(heads_seed(s))
    K = sum(Cs)
    npow = 1
    while npow < ncls:
        npow *= 2
    d = dict(sides=[_ints(rs, (rows, c)) for c in Cs], Wc=_ints(rs, (ncls, K)), bc=_ints(rs, (ncls,)), Ws=_ints(rs, (K,)), bs=_ints(rs, (1,)),
             probs=np.full((rows, ncls), 1.0 / npow, F32), dprobs=_ints(rs, (rows, ncls)), dstop=_ints(rs, (rows,)), npow=npow,
             fill=dict(dWc=_ints(rs, (ncls, K), True), dbc=_ints(rs, (ncls,), True), dWs=_ints(rs, (K,), True), dbs=_ints(rs, (1,), True)))
    sv = np.concatenate(d["sides"], 1).astype(np.float64)
    d["stop"] = sv @ d["Ws"].astype(np.float64) + float(d["bs"][0])
    d["ref"] = heads_bwd64(d["sides"], d["Wc"], d["Ws"], d["probs"], d["dprobs"], d["dstop"])
    return d


def heads_exact_bound(d):
    """the largest sum of |terms| of any output of the exact case, prefill included: the backward's in units of the smallest d-logit
    step 1 / npow^2, the stop logit's in units of 1 (each must stay < 2^24)"""
    sv = np.abs(np.concatenate(d["sides"], 1)).astype(np.float64)
    dl = np.abs(d["ref"]["dl"])
    aw, as_, ads = np.abs(d["Wc"]).astype(np.float64), np.abs(d["Ws"]).astype(np.float64), np.abs(d["dstop"]).astype(np.float64)
    bwd = max((dl @ aw + ads[:, None] * as_[None, :]).max(), (dl.T @ sv).max() + 3, dl.sum(0).max() + 3, (ads @ sv).max() + 3, ads.sum() + 3)
    return max(bwd * d["npow"] ** 2, (sv @ as_).max() + 3)


def heads_normal_data(s, regime):
    """N(0, 1) features, nn.Linear initialisation (uniform +-1 / sqrt(K)); `hot`: fc_class scaled by 256, so the class logits have a
    standard deviation of ~150 and the softmax is saturated (the winner at 1 - 1e-7 or closer, the rest near or below 1e-14).
    Returns the inputs, the float64 references and the host models' errors per output group."""
    rows, Cs, ncls = s
    rs = _rng(heads_seed(s) + (1 if regime == "hot" else 0))
    K = sum(Cs)
    bound = 1.0 / np.sqrt(K)
    sides = [rs.normal(0, 1, (rows, c)).astype(F32) for c in Cs]
    scale = 256.0 if regime == "hot" else 1.0
    Wc, bc = (rs.uniform(-bound, bound, (ncls, K)) * scale).astype(F32), (rs.uniform(-bound, bound, (ncls,)) * scale).astype(F32)
    Ws, bs = rs.uniform(-bound, bound, (K,)).astype(F32), rs.uniform(-bound, bound, (1,)).astype(F32)
    dprobs, dstop = rs.normal(0, 1, (rows, ncls)).astype(F32), rs.normal(0, 1, (rows,)).astype(F32)
    sv = np.concatenate(sides, 1)
    sv64 = sv.astype(np.float64)
    lg = sv64 @ Wc.astype(np.float64).T + bc.astype(np.float64)
    ex = np.exp(lg - lg.max(1, keepdims=True))
    probs64, stop64 = ex / ex.sum(1, keepdims=True), sv64 @ Ws.astype(np.float64) + float(bs[0])
    # host model, forward: one fp32 chain over the K features per logit, bias last; softmax as the kernel's thread 0 forms it
    W_all, b_all = np.concatenate([Wc, Ws[None, :]], 0), np.concatenate([bc, bs])
    acc = np.zeros((rows, ncls + 1), F32)
    for k in range(K):
        acc = acc + sv[:, k, None] * W_all[None, :, k]
    acc = acc + b_all[None, :]
    e32 = np.exp(acc[:, :ncls] - acc[:, :ncls].max(1, keepdims=True), dtype=F32)
    probs32, stop32 = e32 / chain32(e32, 1)[:, None], acc[:, ncls]
    assert probs32.dtype == F32 and stop32.dtype == F32
    # the backward takes probs as an INPUT: the fp32 probabilities of the host model
    ref = heads_bwd64(sides, Wc, Ws, probs32, dprobs, dstop)
    dot = chain32(dprobs * probs32, 1)
    dl32 = np.concatenate([probs32 * (dprobs - dot[:, None]), dstop[:, None]], 1)
    ds32 = dl32[:, ncls, None] * Ws[None, :]
    for c in range(ncls):
        ds32 = ds32 + dl32[:, c, None] * Wc[None, c, :]
    gW = np.zeros((ncls + 1, K), F32)
    gb = np.zeros((ncls + 1,), F32)
    for i in range(rows):
        gW = gW + dl32[i, :, None] * sv[None, i, :]
        gb = gb + dl32[i]
    assert ds32.dtype == F32 and gW.dtype == F32 and gb.dtype == F32
    e = lambda a, r: float(np.abs(a.astype(np.float64) - r).max())
    err_host = dict(probs=e(probs32, probs64), stop=e(stop32, stop64), dside=e(ds32, ref["dside"]),
                    params=max(e(gW[:ncls], ref["dWc"]), e(gW[ncls], ref["dWs"]), e(gb[:ncls], ref["dbc"]), e(gb[ncls:], ref["dbs"])))
    return dict(sides=sides, Wc=Wc, bc=bc, Ws=Ws, bs=bs, probs_in=probs32, dprobs=dprobs, dstop=dstop, probs=probs64, stop=stop64, ref=ref,
                err_host=err_host, host=dict(probs=probs32, stop=stop32, dside=ds32, dW=gW, db=gb))


# ---- the (value, pixel) keys of the fused global max-pool (common.h rsis_side_key / rsis_side_value / rsis_side_index)
def side_key(v, idx):
    u = np.asarray(v, F32).view(np.uint32).astype(np.uint64)
    u = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return (u << np.uint64(32)) | (np.uint64(0x7FFFFFFF) - np.asarray(idx, np.uint64))


def side_key_decode(k):
    k = np.asarray(k, np.uint64)
    u = (k >> np.uint64(32)).astype(np.uint64)
    u = np.where(u & np.uint64(0x80000000), u & np.uint64(0x7FFFFFFF), ~u & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return u.view(F32), (np.uint64(0x7FFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64).astype(np.int32)


F32_MAX = float(np.finfo(F32).max)
KEY_VALUES = np.array([0.0, -0.0, -1.5, -2.0 ** -100, F32_MAX, -F32_MAX, 1e-40, -1e-40, 1.0, 2.0 ** -126], F32)   # (1e-40: a denormal)
KEY_PIXELS = np.array([0, 2 ** 20 - 1, 1, 2 ** 20 - 1, 0, 2 ** 20 - 1, 0, 2 ** 20 - 1, 12345, 0], np.int32)
KEYS_SHAPE = (5, [16, 8, 8], 7)


def keys_data():
    """chosen (value, pixel) pairs in the first columns of level 0 (rotated by the row, so that every row differs), seeded N(0, 1)
    values and pixels below 2^20 elsewhere; weights small enough that +-FLT_MAX features give finite logits"""
    rows, Cs, ncls = KEYS_SHAPE
    rs = _rng(88)
    K = sum(Cs)
    vals = [rs.normal(0, 1, (rows, c)).astype(F32) for c in Cs]
    pix = [rs.integers(0, 2 ** 20, (rows, c)).astype(np.int32) for c in Cs]
    n = len(KEY_VALUES)
    for r in range(rows):
        vals[0][r, :n], pix[0][r, :n] = np.roll(KEY_VALUES, r), np.roll(KEY_PIXELS, r)
    bound = 0.1 / np.sqrt(K)
    return dict(vals=vals, pix=pix, keys=[side_key(v, p) for v, p in zip(vals, pix)],
                Wc=rs.uniform(-bound, bound, (ncls, K)).astype(F32), bc=rs.uniform(-1, 1, (ncls,)).astype(F32),
                Ws=rs.uniform(-bound, bound, (K,)).astype(F32), bs=rs.uniform(-1, 1, (1,)).astype(F32))


# ======================================================================================================================
# 3. loss tail
# ======================================================================================================================
TAIL_N = (1, 30, 255, 256, 257, 320, 1280, 4096)       # the two loops of loss_tail_kernel stride by 256 rows
TAIL_W = (F32(1.0), F32(0.1), F32(0.5))                # w_iou, w_cls, w_stop (args.py defaults), as the fp32 values the C ABI receives
TAIL_BW = F32(0.3)
TAIL_GOUT = F32(1.7)


def _tail_cases():
    """every n in both regimes, the other dimensions cycling; the full cross of C x bw x class weights at n = 320 (the bench's B * T)"""
    cases = []
    Cs = (2, 21, 64)
    for i, n in enumerate(TAIL_N):
        for r, regime in enumerate(("normal", "hot")):
            cases.append(dict(n=n, C=Cs[(i + r) % 3], bw=(i + r) % 2 == 0, cw=(i // 2 + r) % 2 == 0, regime=regime, gout=True))
    for C in Cs:
        for bw in (True, False):
            for cw in (True, False):
                c = dict(n=320, C=C, bw=bw, cw=cw, regime="normal", gout=True)
                if c not in cases:
                    cases.append(c)
    cases.append(dict(n=257, C=21, bw=True, cw=False, regime="normal", gout=False))       # gout null: the upstream gradient is 1
    return cases


def tail_id(c):
    return "n%d_c%d_%s_%s_%s%s" % (c["n"], c["C"], "bw" if c["bw"] else "auto", "cw" if c["cw"] else "nocw", c["regime"], "" if c["gout"] else "_g1")


TAIL_CASES = _tail_cases()
TAIL_MASKING_N = (30, 320, 1280)


def tail_inputs(c):
    n, C = c["n"], c["C"]
    rs = _rng(n * 13 + C * 3 + (1 if c["regime"] == "hot" else 0) + (5 if c["bw"] else 0) + (7 if c["cw"] else 0))
    lg = rs.normal(0, 2, (n, C))
    ex = np.exp(lg - lg.max(1, keepdims=True))
    probs = (ex / ex.sum(1, keepdims=True)).astype(F32)
    y = rs.integers(0, C, (n,)).astype(np.int64)
    hot = c["regime"] == "hot"
    stop = rs.normal(0, 15.0 if hot else 3.0, (n,)).astype(F32)
    siou = rs.random(n).astype(F32)
    swm, swc = (rs.random(n) < 0.6).astype(F32), (rs.random(n) < 0.7).astype(F32)
    swm[0] = swc[0] = 1                                   # each mask keeps a selected row
    if hot:                                               # the target class's probability down to 1e-30, and exactly 1, on selected rows
        sel = np.flatnonzero(swm)
        tiny = (10.0 ** -rs.uniform(0, 30, sel.size)).astype(F32)
        tiny[0] = F32(1e-30)
        for j, i in enumerate(sel):
            if j % 3 == 0:
                probs[i, y[i]] = tiny[j]
            elif j % 3 == 1:
                probs[i, y[i]] = 1.0
    cw = (rs.random(C) + 0.5).astype(F32) if c["cw"] else None
    return dict(probs=probs, y=y, stop=stop, siou=siou, swm=swm, swc=swc, cw=cw, bw=TAIL_BW if c["bw"] else None,
                gout=TAIL_GOUT if c["gout"] else None)


def tail_eval(q, dt):
    """train.py:159-176 with hungarian.py:10-59 on the n rows, every operation in dtype dt (float64: the reference; float32: the host
    model, its masked sums sequential chains over the selected rows in row order), and the gradients of the total times gout.
    Returns (out[4] = total, iou, stop, class; dprobs, dstop, dsiou; coef = |gout w_stop / sum_c * bal| per row)."""
    f = dt
    n, C = q["probs"].shape
    w_iou, w_cls, w_stop = (f(w) for w in TAIL_W)
    gout = f(q["gout"]) if q["gout"] is not None else f(1)
    t, wm, wc = q["swm"].astype(f), q["swm"] > 0, q["swc"] > 0
    p = q["probs"][np.arange(n), q["y"]].astype(f)
    cw = q["cw"].astype(f)[q["y"]] if q["cw"] is not None else np.ones(n, f)
    x = q["stop"].astype(f)
    sum_m, sum_c = f(wm.sum()), f(wc.sum())
    bw = f(q["bw"]) if q["bw"] is not None else f(wm.sum()) / f(n)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        nll = -np.log(p) * cw
        mx = np.maximum(-x, f(0))
        lv = x - x * t + mx + np.log(np.exp(-mx) + np.exp(-x - mx))
        bal = (f(1) - bw) * t + bw * (f(1) - t)
        summ = (lambda a: chain32(a)) if f is F32 else (lambda a: a.sum())
        l_iou, l_cls, l_stop = summ(q["siou"].astype(f)[wm]) / sum_m, summ(nll[wm]) / sum_m, summ((lv * bal)[wc]) / sum_c
        out = np.array([w_iou * l_iou + w_cls * l_cls + w_stop * l_stop, l_iou, l_stop, l_cls], f)
        dsiou = np.where(wm, gout * w_iou / sum_m, f(0))
        coef = gout * w_stop / sum_c * bal
        dstop = np.where(wc, coef * (f(1) / (f(1) + np.exp(-x)) - t), f(0))
        dprobs = np.zeros((n, C), f)
        dprobs[np.arange(n), q["y"]] = np.where(wm, -gout * w_cls * cw / (sum_m * p), f(0))
    assert out.dtype == f and dstop.dtype == f and dprobs.dtype == f
    return dict(out=out, dprobs=dprobs, dstop=dstop, dsiou=dsiou, coef=np.where(wc, np.abs(coef), f(0)), sums=(float(sum_m), float(sum_c)))


def tail_auto_bw(q):
    return float(q["swm"].sum()) / q["swm"].size


# elementwise gradients of the loss tail, roundings in units of 2^-24 (sum_m, sum_c, t are exact):
#   dsiou  = gout * w_iou / sum_m                          : product, division                                               -> 2
#   dprobs = -gout * w_cls * cw / (sum_m * p)              : three products, division                                        -> 4
#   dstop  = gout * w_stop / sum_c * bal * (sigmoid(x) - t): coef = product, division (2); bal = (1 - bw) t + bw (1 - t) is 1 - bw or bw:
#            bw itself (auto: npos / n) 1, and 1 - bw carries u bw / (1 - bw) + u <= 4 u for bw <= 3 / 4 (or bw = 1: exactly 0) -> 4;
#            sigmoid 4 as in K_DLOGITS; the subtraction 1; the two products 2                                               -> 13, relative,
#            and sigmoid's ABSOLUTE error 4 u against a difference that cancels: + 13 u |coef| (coef = gout w_stop / sum_c * bal)
K_DSIOU, K_DPROBS, K_DSTOP = 2, 4, 13
TAIL_MAX_AUTO_BW = 0.75


# ======================================================================================================================
# 4. assignment
# ======================================================================================================================
ASSIGN_SIZES = [(1, 1), (20, 10), (7, 7), (64, 64), (64, 1), (65, 65), (65, 1), (128, 128), (100, 64), (127, 33)]     # (G, T)
ASSIGN_STRUCTS = ("train", "dup", "quarters", "const")
ASSIGN_B = 3
Q20 = 2.0 ** 20


def q20(a):
    """quantise to multiples of 2^-20 (exact in fp32 below 16; float64 totals of <= 128 of them and the kernels' fp64 potentials are exact)"""
    return (np.floor(np.asarray(a, np.float64) * Q20) / Q20).astype(F32)


def assign_scores(G, T, struct):
    """(3, G, T) fp32 scores, rows = GT slots, columns = predictions"""
    rs = _rng(G * 1000 + T * 7 + ASSIGN_STRUCTS.index(struct))
    B = ASSIGN_B
    if struct == "train":
        # train.py:173-181: costs in [0, 1] with many exact 1.0 (empty GT slots, empty predictions), 1.0 in every column >= t (steps not
        # run), 10 on invalid pairs: image 0 has every slot valid, image 1 n_inst = T // 2 < T instances, image 2 none at all
        s = q20(rs.random((B, G, T)))
        s[rs.random((B, G, T)) < 0.4] = 1.0
        s[:, :, max(1, T - T // 4):] = 1.0
        for b, n_inst in ((1, T // 2), (2, 0)):
            sw = (np.arange(G) < n_inst).astype(F32)
            valid = sw[:, None] * sw[None, :T]
            s[b] = s[b] * valid + (1 - valid) * 10
    elif struct == "dup":
        # predictions that coincide (duplicated columns) and GT instances that coincide (duplicated rows): ties everywhere
        base = q20(rs.random((B, (G + 1) // 2, (T + 1) // 2)))
        s = np.repeat(np.repeat(base, 2, 1), 2, 2)[:, :G, :T].copy()
    elif struct == "quarters":
        s = (rs.integers(0, 5, (B, G, T)) / 4.0).astype(F32)
    else:
        s = np.stack([np.full((G, T), v, F32) for v in (0.5, 1.0, 10.0)])
    return np.ascontiguousarray(s, dtype=F32)


def assign_optimum(s):
    """scipy's optimum total per image, float64 (exact for q20 scores)"""
    from scipy.optimize import linear_sum_assignment
    tot = []
    for b in range(s.shape[0]):
        S = s[b].astype(np.float64)
        r, c = linear_sum_assignment(S)
        tot.append(S[r, c].sum())
    return np.array(tot)


def assign_sequential(s):
    """The algorithm of assign_kernel / assign2_kernel run sequentially in float64: shortest augmenting paths with potentials, rows =
    predictions taken in order, the scan over the GT slots keeps the FIRST minimum.  With q20 scores every potential is exact, so the
    kernels' perm must EQUAL this one -- which optimum they return among tied ones is then pinned as well (the wave arg-min's "smallest
    lane on ties", assign2's "column < 64 first")."""
    B, G, T = s.shape
    perm = np.zeros((B, G), np.int64)
    for b in range(B):
        a = s[b].astype(np.float64).T                     # a[prediction][slot]
        u, v = np.zeros(T + 1), np.zeros(G + 1)
        p, way = np.zeros(G + 1, np.int64), np.zeros(G + 1, np.int64)
        for i in range(1, T + 1):
            p[0], j0 = i, 0
            minv, used = np.full(G + 1, np.inf), np.zeros(G + 1, bool)
            while True:
                used[j0] = True
                i0 = p[j0]
                cur = a[i0 - 1] - u[i0] - v[1:]
                upd = ~used[1:] & (cur < minv[1:])
                minv[1:][upd], way[1:][upd] = cur[upd], j0
                cand = np.where(used[1:], np.inf, minv[1:])
                j1 = int(np.argmin(cand)) + 1              # the first minimum
                delta = cand[j1 - 1]
                u[p[used]] += delta
                v[used] -= delta
                minv[~used] -= delta
                j0 = j1
                if p[j0] == 0:
                    break
            while j0:
                j1 = way[j0]
                p[j0] = p[j1]
                j0 = j1
        for j in range(1, G + 1):
            if p[j]:
                perm[b, p[j] - 1] = j - 1
    return perm


def assign_total(s, perm):
    """float64 total of the assignment perm[b][t] = GT slot of prediction t"""
    T = s.shape[2]
    return np.array([s[b].astype(np.float64)[perm[b, :T], np.arange(T)].sum() for b in range(s.shape[0])])


# ======================================================================================================================
# margins: TWICE the worst err_gpu / err_host measured on the MI355X over every normal case and both modes
# (profiles/r14_a_loss_path_margins.txt, NOTES.md (88)); each must stay <= 4
# ======================================================================================================================
M_IOU = 2.19      # 2 x 1.091: b2_t5_g31_n72, N(0, 2), deterministic mode (one wave per image: the MFMA's own chain against the host's)
M_HEADS = 2.56    # 2 x 1.278: the parameter gradients of r97_k16+8_c33 (fmaf chain over the rows against the host's mul + add chain)
M_TAIL = 4.0      # the cap, not 2 x a ratio: the worst ratios are 3.73 and 3.22 (class NLL mean at n = 320), all others <= 1.52 -- see test_loss_tail
