"""Shapes, keys and host references shared by the dropout tests (test_dropout_host.py, test_gpu_dropout.py)."""
import numpy as np

from rsis_amd import dropout as D

HS, T, B = 128, 3, 2
HIDS = [HS, HS // 2, HS // 4, HS // 8, HS // 16]
CHANS = [HS, HS, HS // 2, HS // 4, HS // 8]          # skip-feature channels per level
SIZES = {
    "pow2": [(2, 2), (4, 4), (8, 8), (16, 16), (32, 32)],
    "odd": [(3, 4), (5, 7), (10, 13), (19, 25), (37, 50)],            # the shapes of the dec_odd fixture
    "same": [(3, 4), (6, 8), (6, 8), (12, 16), (12, 16)],              # levels 1 -> 2 and 3 -> 4: the equal-size (copy) case
}
SEED = 0x5EED1234          # key word 0 of every state the GPU tests start from (key word 1: rank 0)


def state0(rank=0):
    return [SEED, rank, 0, 0]


def n_elems(T=T, B=B):
    return T * B * sum(HIDS)


def per_level(flat, T=T, B=B):
    """[n] -> per level [T][B][hid] (the layout of the decoder's pooled features)"""
    out, o = [], 0
    for h in HIDS:
        out.append(flat[o:o + T * B * h].reshape(T, B, h))
        o += T * B * h
    return out


def masks(state, rates, T=T, B=B):
    """(s2, mc, ms) as rsis_dropout_scales fills them at `state`, flat float32"""
    n = n_elems(T, B)
    return [D.scales_numpy(state, a, n, p) for a, p in zip((D.ARRAY_S2, D.ARRAY_MC, D.ARRAY_MS), rates)]


def nondegenerate(flat, T=T, B=B):
    """every (level, b) holds at least one kept and one dropped entry"""
    return all(bool((lv[:, b] > 0).any()) and bool((lv[:, b] == 0).any()) for lv in per_level(flat, T, B) for b in range(B))
