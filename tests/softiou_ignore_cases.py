"""Cases, input builders and the float64 statement of the soft-IoU kernels WITH AN IGNORE REGION (rsis_softiou_sums_ignore /
rsis_softiou_bwd_ignore, csrc/losses.hip) for test_gpu_softiou_ignore.py, checked without a device by test_ignore_host.py.  Numpy on the
host; nothing imports the library.  The shapes are those of loss_path_cases.py that cross each launch rule.

Definition (include/rsis_hip.h): ignore[b][n] one byte per pixel, k = (ignore == 0), p = sigmoid(logit):
    I[t][g] = sum_n k p_t y_g      P[t] = sum_n k p_t      Y[g] = sum_n k y_g      cost = 1 - I / (P + Y - I + 1e-6)
    d cost / d logit_n = k_n (ca y + cb (1 - y)) p (1 - p)
The ground-truth masks built here hold ONES inside every ignored pixel, in every slot, so that a kernel which trusts the loader to
have cleared them (and does not mask Y itself) misses every sum of the column."""
import numpy as np

import loss_path_cases as L

F32 = np.float32

ONES_IDS = ("b2_t1_g1_n8", "b2_t31_g5_n72", "b2_t5_g31_n72", "b1_t31_g31_n520", "b3_t10_g20_n4096")
TILED_IDS = ("b2_t32_g1_n64", "b2_t1_g32_n64", "b1_t33_g33_n520", "b1_t65_g127_n136", "b1_t128_g128_n520")


def _pick(ids, pool):
    by = {L.iou_id(c): c for c in pool}
    return [by[i] for i in ids]


IGN_ONES = _pick(ONES_IDS, L.IOU_ONES)
IGN_TILED = _pick(TILED_IDS, L.IOU_TILED)
IGN_CASES = IGN_ONES + IGN_TILED
IGN_BWD_ONLY = list(L.IOU_BWD_ONLY)                  # N = 1048576, T = 9, G = 3: the grid-stride loop's second trip
# a normal case is judged by the largest error over its sums: the rule of loss_path_cases.IOU_NORMAL (enough summed terms behind it)
IGN_NORMAL = [c for c in IGN_CASES if L.iou_population(c) * c["N"] >= L.MIN_TERMS]
PATTERNS = ("zero", "ones", "p30", "step", "image")


def ignore_map(c, pattern):
    """(B, N) uint8.  zero / ones: nothing / everything ignored; p30: seeded, 30 % of the pixels, with values 1..255 (any non-zero byte
    ignores); step: every pixel of ONE 8-pixel step per image (pixels 8 s .. 8 s + 7, s the image's own: a whole MFMA step of the wave
    that walks it contributes nothing); image: image 0 ignored everywhere, the others not at all."""
    B, N = c["B"], c["N"]
    rs = L._rng(L.iou_seed(c) + 7919 + PATTERNS.index(pattern))
    ign = np.zeros((B, N), np.uint8)
    if pattern == "ones":
        ign[:] = 1
    elif pattern == "p30":
        ign[:] = np.where(rs.random((B, N)) < 0.3, rs.integers(1, 256, (B, N)), 0).astype(np.uint8)
    elif pattern == "step":
        for b in range(B):
            s = int(rs.integers(0, N // 8))
            ign[b, 8 * s:8 * s + 8] = 1
    elif pattern == "image":
        ign[0] = 1
    elif pattern != "zero":
        raise ValueError(pattern)
    return ign


def keep64(ignore):
    return (np.asarray(ignore) == 0).astype(np.float64)


def sums64_ignore(p, y, ignore):
    """S (B, T+1, G+1) float64 of the definition: probabilities p (B, T, N), masks y (B, G, N), ignore (B, N)"""
    k = keep64(ignore)[:, None, :]
    return L.sums64(np.asarray(p, np.float64) * k, np.asarray(y, np.float64) * k)


def sums_chain32_ignore(logits, y, ignore):
    """the host model over the masked terms: fp32 sigmoid, fp32 products, the factor k (exact), one sequential fp32 chain per sum"""
    k = (np.asarray(ignore) == 0).astype(F32)
    p = L.sigmoid32(logits) * k[:, None, :]
    yk = np.asarray(y, F32) * k[:, None, :]
    B, T, N = p.shape
    G = yk.shape[1]
    S = np.zeros((B, T + 1, G + 1), F32)
    for b in range(B):
        for t in range(T):
            S[b, t, :G] = L.chain32(p[b, t][None, :] * yk[b])
        S[b, :T, G] = L.chain32(p[b])
        S[b, T, :G] = L.chain32(yk[b])
    return S


def bwd64_ignore(logits, y, ignore, perm, ca, cb, p=None):
    return L.iou_bwd64(logits, y, perm, ca, cb, p) * keep64(ignore)[:, None, :]


def _masks(rs, c, ign):
    y = L._iou_masks(rs, c["B"], c["G"], c["N"])
    y[np.broadcast_to((ign != 0)[:, None, :], y.shape)] = 1          # ones under every ignored pixel, in every slot
    return y


def exact_data(c, pattern, with_sums=True):
    """loss_path_cases.iou_exact_data with the map: logits from EXACT_LOGITS, integer ca / cb; sums are counts in halves"""
    B, T, G, N = c["B"], c["T"], c["G"], c["N"]
    rs = L._rng(L.iou_seed(c))
    ign = ignore_map(c, pattern)
    logits = np.array(L.EXACT_LOGITS, F32)[rs.integers(0, 3, (B, T, N))]
    y = _masks(rs, c, ign)
    perm = L._iou_perm(rs, B, T, G)
    ca = rs.integers(-3, 4, (B, T)).astype(F32)
    cb = rs.integers(-3, 4, (B, T)).astype(F32)
    d = dict(logits=logits, y=y, ignore=ign, perm=perm, ca=ca, cb=cb)
    if with_sums:
        d["S"] = sums64_ignore(L.sigmoid32(logits), y, ign)
    d["dlogits"] = bwd64_ignore(logits, y, ign, perm, ca, cb, L.sigmoid32(logits))
    return d


def normal_data(c, regime, pattern):
    """loss_path_cases.iou_normal_data with the map: seeded N(0, scale) logits, float64 references, the host model's error"""
    B, T, G, N = c["B"], c["T"], c["G"], c["N"]
    rs = L._rng(L.iou_seed(c) + (1 if regime == "hot" else 0))
    ign = ignore_map(c, pattern)
    logits = rs.normal(0, L.IOU_REGIMES[regime], (B, T, N)).astype(F32)
    y = _masks(rs, c, ign)
    perm = L._iou_perm(rs, B, T, G)
    S = sums64_ignore(L.sigmoid64(logits), y, ign)
    err_host = float(np.abs(sums_chain32_ignore(logits, y, ign).astype(np.float64) - S).max())
    cost, den = L.cost64(S)
    ca = rs.normal(0, 1, (B, T)).astype(F32) / F32(N)
    cb = rs.normal(0, 1, (B, T)).astype(F32) / F32(N)
    return dict(logits=logits, y=y, ignore=ign, perm=perm, S=S, err_host=err_host, cost=cost, den=den, ca=ca, cb=cb,
                dlogits=bwd64_ignore(logits, y, ign, perm, ca, cb))


def matched_grad64(logits, y, ignore, perm, g, e=1e-6):
    """float64 gradient of sum_bt g[b][t] * cost[b][t] (the matched pairs (perm[b][t], t)) w.r.t. the logits, and the pieces the bar of
    the autograd test needs: (dlogits, U (B, T), coef (B, T) = max(|ca|, |cb|))"""
    B, T, _ = logits.shape
    S = sums64_ignore(L.sigmoid64(logits), y, ignore)
    G = y.shape[1]
    bi, ti = np.arange(B)[:, None], np.arange(T)[None, :]
    gi = perm[:, :T]
    inter = S[:, :T, :G][bi, ti, gi]
    U = S[:, :T, G] + S[:, T, :G][bi, gi] - inter + e
    ca, cb = -g / U, g * inter / (U * U)
    d = L.iou_bwd64(logits, y, perm, ca, cb) * keep64(ignore)[:, None, :]
    return d, U, np.maximum(np.abs(ca), np.abs(cb))


# the margin of the normal-regime sums: TWICE the worst err_gpu / err_host measured on the MI355X over IGN_NORMAL x both regimes x every
# pattern x both modes; it must stay <= 4 (the rule of loss_path_cases.M_IOU, NOTES.md (88)).
# (profiles/r21_a_ignore_margins.txt, NOTES.md (98)): the worst ratios all sit at N = 72, where a sum has at most 72 terms and err_host is
# one or two roundings of the host chain.
M_IOU_IGN = 3.43     # 2 x 1.714: b2_t5_g31_n72, N(0, 2), seeded 30 % map, both modes (next: 1.436, b2_t31_g5_n72, one image ignored)
