"""Case tables and float64 references of the `-skip_mode sum | mul | none` tests (test_skip_modes_host.py on the host,
test_gpu_skip_modes.py on the GPU).  Plain data and pure functions: nothing here touches the GPU.

  PACK_OFFSETS   the gate-weight columns of decoder_fused._packs per mode, restated as data
  CHANNEL_RULE   the per-mode channel rule of decoder_seq.supported
  mul kernels    y = resize_ac(x) * m and its backward preparation in float64, with the a-priori bars of resample_cases.py
  fma32          fp32 fused multiply-add on the host, correctly rounded (the accumulate form of the preparation kernels)"""
import numpy as np

import resample_cases as R

MODES = ("concat", "sum", "mul", "none")
U = R.U

# (mode, c_up, c_skip) -> (first column of the hoisted skip term or None, first column of h_prev); reference model.py:98-106,151-158:
# concat: x = [up | skip]; sum / mul: x has c_up channels; none: x = up.  Level 0 (c_up == 0) takes its skip feature alone in every mode.
PACK_OFFSETS = {
    ("concat", 64, 64): (64, 128), ("concat", 16, 32): (16, 48), ("concat", 0, 128): (0, 128),
    ("sum", 64, 64): (0, 64), ("sum", 8, 8): (0, 8), ("sum", 0, 128): (0, 128),
    ("mul", 64, 64): (None, 64), ("mul", 8, 8): (None, 8), ("mul", 0, 128): (0, 128),
    ("none", 64, 64): (None, 64), ("none", 16, 32): (None, 16), ("none", 0, 128): (0, 128),
}

# (mode, input_size, c_up, c_skip) -> does the sequence node take the level
CHANNEL_RULE = [
    ("concat", 128, 64, 64, True), ("concat", 64, 64, 64, False), ("concat", 128, 0, 128, True),
    ("sum", 64, 64, 64, True), ("sum", 128, 64, 64, False), ("sum", 64, 64, 32, False), ("sum", 128, 0, 128, True),
    ("mul", 64, 64, 64, True), ("mul", 64, 64, 32, False), ("mul", 96, 64, 32, False), ("mul", 128, 0, 128, True),
    ("none", 64, 64, 64, True), ("none", 64, 64, 32, True), ("none", 128, 64, 64, False), ("none", 128, 0, 128, True),
    ("bogus", 64, 64, 64, False),
]


def level_channels(hidden, mode):
    """(input_size, c_up, c_skip) of the five levels of the reference's pyramid (model.py:91-106) for a hidden size"""
    hs = [hidden, hidden // 2, hidden // 4, hidden // 8, hidden // 16]
    skip = [hidden, hidden, hidden // 2, hidden // 4, hidden // 8]
    out = []
    for i in range(5):
        c_up = 0 if i == 0 else hs[i - 1]
        cin = hidden if i == 0 else (2 * hs[i - 1] if mode == "concat" else hs[i - 1])
        out.append((cin, c_up, skip[i]))
    return out


# ---------------------------------------------------------------- fp32 kernels: the cases
def smallest_per_path():
    """one case of resample_cases.UP_FWD per launch path of the fp32 resize, the one with the fewest outputs, and both identity cases"""
    best = {}
    for c in R.UP_FWD:
        n = c["BC"] * c["Ho"] * c["Wo"]
        if c["path"] not in best or n < best[c["path"]][0]:
            best[c["path"]] = (n, c)
    out = [c for _n, c in best.values()]
    out += [c for c in R.UP_FWD if c.get("identity") and all(c is not d for d in out)]
    return out


MUL_FWD = smallest_per_path()
# the preparation kernel has two paths of its own: rows of whole float4s (wherever the forward runs an LDS or a v4 kernel) and the
# forward's scalar loop.  On the scalar path u has the scalar kernel's bits for every element a thread computes in the LAST trip of its
# grid-stride loop -- all of them up to 2^20 elements per launch, the sizes below (that kernel rounds a thread's earlier trips in pairs,
# with another contraction of the same blend; see NOTES.md (96))
MUL_PREP = [c for c in MUL_FWD if c["BC"] * c["Ho"] * c["Wo"] <= R.TWO20]


def mul_operands(c, n=1):
    """m and n gradients dy of a case (fp32, y's shape), from its seed"""
    rs = np.random.default_rng(R.case_seed(c) + 77)
    shape = (c["BC"], c["Ho"], c["Wo"])
    m = rs.normal(0, 1, shape).astype(np.float32)
    return m, [rs.normal(0, 1, shape).astype(np.float32) for _ in range(n)]


def mul_fwd_ref(c, m):
    """(want, bar) in float64: F.interpolate(x, align_corners=True) * m; the unscaled kernel's bar against that reference times |m|,
    plus one fp32 rounding of the product"""
    r = R.up_fwd_refs(c)
    m64 = m.astype(np.float64)
    want = r["ref"] * m64
    bar = r["bar_ref"] * np.abs(m64)
    return want, bar + U * (np.abs(want) + bar)


def mul_prep_ref(c, m, dy):
    """float64 statement of the preparation in store mode: (dy * m, dy * resize(x))"""
    r = R.up_fwd_refs(c)
    return dy.astype(np.float64) * m.astype(np.float64), dy.astype(np.float64) * r["ref"]


# ---------------------------------------------------------------- fp32 fma on the host
def fma32(a, b, c):
    """round_fp32(a * b + c) of fp32 arrays with ONE rounding: the product of two fp32 numbers is exact in float64; the float64 sum is
    turned into a round-to-odd result with the exact residual of TwoSum, after which the rounding to fp32 cannot double-round (53 >= 24 + 2)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)             # exact: p + c = s + err
    bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
    even = (bits & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


# ---------------------------------------------------------------- the decoder cases
HS = 32
PYRAMID = [(2, 3), (4, 6), (8, 12), (16, 24), (32, 48)]
PYRAMID_SAME = [(2, 3), (4, 6), (4, 6), (8, 12), (16, 24)]        # levels 1 -> 2: the identity resize
BLK_HS = 128
BLK_PYRAMID = [(2, 2), (4, 4), (7, 7), (14, 14), (28, 28)]


def skip_channels(hidden):
    return [hidden, hidden, hidden // 2, hidden // 4, hidden // 8]
