"""The dropout of the recurrent decoder (`-dropout`, `-dropout_cls`, `-dropout_stop`; reference model.py:137-182) on the one-node
sequence decoder: scales drawn ONCE per sequence by a counter-based generator on the device (rsis_dropout_scales, csrc/dropout.hip) and
folded into the launches rsis_amd.decoder_seq makes anyway.

Three arrays, all in the layout of the decoder's pooled side features (level after level, each [T][B][hid_i]):
  s2 : the Dropout2d factor of hidden state h[i][t][b][c], 0 or 1 / (1 - p) -- one per channel plane;
  mc, ms : the element masks of the class / stop head features (the concatenation over the levels of row (t, b)).

The rule by which the device fills them is stated in include/rsis_hip.h next to rsis_dropout_scales; `scales_numpy` restates it, so a test
(or a user) can replay any mask from the 4 state words it was drawn at.
"""
import os

import numpy as np
import torch

from ._lib import check, lib, ptr, stream

STATE_WORDS = 8
ARRAY_S2, ARRAY_MC, ARRAY_MS = 0, 1, 2

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).  counter: 4 words, key: 2
    words, each an int or an array of them (broadcast); returns the 4 output words as uint64 arrays holding 32-bit values"""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _MASK for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k[0]) & _MASK, p1 & _MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k[1]) & _MASK, p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return c


def scales_numpy(state, array, n, p):
    """what rsis_dropout_scales writes to array `array` (ARRAY_S2 / _MC / _MS) of n elements at rate p when it finds the words `state`
    (key0 = seed, key1 = rank, call counter low, high): float32 [n]"""
    state = [int(v) & _MASK for v in state[:4]]
    e = np.arange(n, dtype=np.uint64)
    w = philox4x32_10((e >> np.uint64(2), array, state[2], state[3]), (state[0], state[1]))
    word = np.choose((e & np.uint64(3)).astype(np.int64), [np.broadcast_to(x, e.shape) for x in w])
    u = (word >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    p = np.float32(p)
    keep = np.float32(1.0) / (np.float32(1.0) - p)
    return np.where(u >= p, keep, np.float32(0.0)).astype(np.float32)


def advance(state):
    """the state words after one rsis_dropout_scales call"""
    s = [int(v) & _MASK for v in state[:4]]
    c = ((s[3] << 32) | s[2]) + 1
    return [s[0], s[1], c & _MASK, (c >> 32) & _MASK]


def process_rank():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank()
    return int(os.environ.get("RANK", "0"))


def new_state(device, seed=None, rank=None):
    """the generator state of one decoder: 8 int32 device words (key0 = seed, key1 = rank, call counter = 0, the kernel's ticket, 3
    unused).  seed None: 32 bits from torch's (seeded) CPU generator"""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 32, (1,), dtype=torch.int64))
    if rank is None:
        rank = process_rank()
    words = np.array([seed & _MASK, rank & _MASK, 0, 0, 0, 0, 0, 0], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(words.copy()).to(device)


def state_words(state):
    """the 4 words that determine the next draw, as Python ints (synchronises)"""
    return [int(v) & _MASK for v in state[:4].cpu().tolist()]


def decoder_state(decoder, device):
    """the state a decoder with any rate above 0 owns: a plain attribute (no state_dict key), made when first asked for"""
    st = decoder.__dict__.get("_drop_state")
    if st is None or st.device != device:
        st = new_state(device)
        decoder.__dict__["_drop_state"] = st
    return st


def rates(decoder):
    return float(decoder.dropout), float(decoder.dropout_cls), float(decoder.dropout_stop)


def draw(state, n, p2, pc, ps):
    """(s2, mc, ms): three fp32 [n] device arrays from ONE launch, which also advances the state's call counter"""
    out = torch.empty((3, n), dtype=torch.float32, device=state.device)
    check(lib().rsis_dropout_scales(ptr(state), ptr(out[0]), ptr(out[1]), ptr(out[2]), n, p2, pc, ps, stream()), "rsis_dropout_scales")
    return out[0], out[1], out[2]
