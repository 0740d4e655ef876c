"""The T-step recurrent decoder as ONE autograd node with an explicit back-propagation through time.

What it computes is the loop of reference train.py:85-94 / test.py:37-38 around RSIS.forward (model.py:122-184) from the zero
state: per timestep five ConvLSTM levels (clstm.py:19-62), the global max-pool side features (model.py:143), the align-corners
upsamples between levels (:149-150, :163-164), conv_out (:167) and the class / stop heads (:169-182).

`decoder_fused.decoder_sequence` already walks the (level, timestep) grid by diagonals in the FORWARD pass (cell (i, t) needs
up(h[i-1][t]) and (h, c)[i][t-1], so the cells of a diagonal d = i + t are independent and their gate kernels go out as one
grouped launch), but leaves the backward to autograd: one node per cell, run one by one.  Here the backward is written out:

  * the reverse wavefront -- cell (i, t) needs d(up[i+1][t]) from cell (i+1, t) and (dh, dc) through the recurrence from cell
    (i, t+1), both on diagonal d + 1 -- so per diagonal there are three grouped steps: the gradient of every hidden state
    through its upsample + side max-pool, the LSTM pointwise backward, the data gradient of the gate conv;
  * everything that is independent of the recurrence runs ONCE over all T timesteps: conv_out forward / data gradient / weight
    gradient on the stacked [T][B] images (rsis_conv_out_seq_*: 3 launches instead of 3 T), the mask logits written straight into
    the (B, T, N) layout train.py:118 stacks them into, the sum over t of d(gates) for the time-invariant skip term
    (rsis_sum_leading), the time-batched weight gradients of the recurrent channels (as decoder_fused does).

The schedule is written once, in _DecoderSeqFn.  How the recurrence is stored is a layout object the node asks for buffers and
launches, picked per call by blk_supported():

  * _Nchw: fp32 NCHW (-dtype fp32, and -dtype bf16 under RSIS_DECODER_BLK=0);
  * _Blk: channel-blocked bf16 [B][C/8][H][W][8] for hidden states, saved gates, up-sampled inputs, the hoisted gate terms and
    their gradients (-dtype bf16); the cell state and its gradient stay fp32 NCHW in both.

Arithmetic and kernels per cell are those of the per-step path (tests/test_gpu_modules.py compares them); only the launch
schedule differs.  The per-timestep `RSIS.forward` stays for callers that thread the state themselves.

`-skip_mode` (model.py:151-158) changes how up = up(h[i-1][t]) meets skip[i] in front of the gate conv of levels 1-4 (_Level.mode):
  * concat: [up | skip | h]; the skip columns are hoisted (G);
  * sum: the conv is linear, conv(up + skip, W_x) = conv(up, W_x) + conv(skip, W_x) -- the concat schedule with the hoisted pack and the
    dynamic up segment both on columns [0, c_up) (decoder_fused.pack_offsets);
  * none: no hoisted term (G, hoist are None): the gate launches take the bias instead of the addend, skip[1..4] get no gradient;
  * mul: as none, and UP[i][t] holds the product up * skip (the mul form of the upsample launches); the backward runs one preparation
    launch in front of the unchanged upsample transposes: DM[i] (+)= dUP * up, dUP <- dUP * skip, DM an fp32 NCHW accumulator that is the
    skip feature's gradient after the last step.  `-dropout > 0` with mul stays on the per-step path (supported()).
"""
import os

import torch

from . import _lib, decoder_fused, dropout, ops
from ._lib import check, int_array, lib, ptr, ptr_array, stream

ENABLED = [os.environ.get("RSIS_DECODER_SEQ", "1") != "0"]
# test hook: RECORD[0] = True keeps a copy of the arg-max pixels of the side max-pools of the last sequence in LAST["arg"] (per level,
# [T][B][hid] int32) -- what the per-step path's callers can read off the returned hidden states -- and, when any dropout rate is above 0,
# clones of the scales the sequence drew in LAST["drop"] = {"s2": per level [T][B][hid] (None at -dropout 0), "mc", "ms": per level
# [T][B][hid]: the head masks of row (t, b) are the concatenation over the levels}
RECORD, LAST = [False], {}


def _is_blk(t):
    return t.dtype == torch.bfloat16 and t.dim() == 5 and t.shape[-1] == 8


def _chan(t):
    """channels of a skip feature given as fp32 NCHW or as a blk tensor [B][C/8][H][W][8]"""
    return t.shape[1] * 8 if _is_blk(t) else t.shape[1]


def supported(decoder, skip_feats, T):
    """the explicit sequence covers the product configuration: the four skip modes, 3x3 gates, any dropout rates in [0, 1) (`-skip_mode mul`:
    -dropout 0 only), the fused heads kernel"""
    n = len(decoder.clstm_list)
    mode = decoder.skip_mode
    if not (ENABLED[0] and decoder_fused.WAVEFRONT[0] and decoder_fused.FUSED_POOL[0] and decoder.fused and mode in decoder_fused.SKIP_MODES and
            len(skip_feats) == n and T >= 1 and "forward" not in decoder.__dict__):
        return False
    if not all(0 <= p < 1 for p in dropout.rates(decoder)):
        return False
    if mode == "mul" and dropout.rates(decoder)[0] > 0:       # (s2 * up(h)) * skip: no launch of the node forms it
        return False
    if not all(f.is_cuda and ((f.dtype == torch.float32 and f.dim() == 4) or _is_blk(f)) for f in skip_feats):
        return False
    if any(_is_blk(f) for f in skip_feats) and not blk_supported(decoder, skip_feats):
        return False
    if not all(c.kernel_size == 3 and c.padding == 1 for c in decoder.clstm_list):
        return False
    if decoder.conv_out.kernel_size != 3 or decoder.conv_out.padding != 1 or decoder.conv_out.bias is None:
        return False
    hs = [c.hidden_size for c in decoder.clstm_list]
    if sum(hs) != decoder.fc_class.weight.shape[1] or not ops.heads_supported([skip_feats[0]] * n, decoder.fc_class, decoder.fc_stop, min_rows=1):
        return False
    for i, c in enumerate(decoder.clstm_list):      # the channel pyramid of model.py:98-106,151-158, per mode
        c_up = 0 if i == 0 else hs[i - 1]
        if not channels_ok(mode, c.input_size, c_up, _chan(skip_feats[i])):
            return False
    return True


def channels_ok(mode, input_size, c_up, c_skip):
    """the input channels of a level's cell: level 0 (c_up == 0) takes its skip feature alone; above it up | skip (concat), up + skip or
    up * skip (sum, mul: equal channel counts), up (none)"""
    if c_up == 0 or mode == "concat":
        return input_size == c_up + c_skip
    if mode in ("sum", "mul"):
        return input_size == c_up == c_skip
    return mode == "none" and input_size == c_up


class ShapeProbe(object):
    """stands in for a skip feature (blk: [B][C/8][H][W][8] bf16, else fp32 NCHW) where only its shape / dtype are consulted: lets the
    callers ask supported() BEFORE the encoder has run (train._blk_skips_ok)"""

    def __init__(self, B, C, H, W, blk):
        self.is_cuda = True
        self.dtype = torch.bfloat16 if blk else torch.float32
        self.shape = (B, C // 8, H, W, 8) if blk else (B, C, H, W)

    def dim(self):
        return len(self.shape)


def supported_for_input(decoder, skip_channels, B, H, W, T):
    """supported() for the skip features a (B, 3, H, W) input will produce when the encoder hands sk5..sk2 over as blk tensors and sk1
    as fp32 NCHW: THE decision whether runIter / test() ask the encoder for blk skip features -- the same predicate the sequence node
    applies afterwards, so the two cannot disagree."""
    sizes, h, w = [], H, W
    for _ in range(5):                      # stem / max-pool / strided 3x3 convs: every halving is ceil(n / 2)
        h, w = (h + 1) // 2, (w + 1) // 2
        sizes.append((h, w))
    sizes = sizes[::-1]                     # x5 .. x1
    if any(c % 8 for c in skip_channels[:4]):
        return False
    probes = [ShapeProbe(B, c, hh, ww, i < 4) for i, (c, (hh, ww)) in enumerate(zip(skip_channels, sizes))]
    return supported(decoder, probes, T) and blk_supported(decoder, probes)


# RSIS_DECODER_BLK=0: keep fp32 NCHW storage in the decoder under -dtype bf16 (bf16 operands only, the round-3 path)
BLK_ENABLED = [os.environ.get("RSIS_DECODER_BLK", "1") != "0"]


def blk_supported(decoder, skip_feats):
    """the decoder's storage half of `-dtype bf16`: every tensor of the recurrence as channel-blocked bf16 (csrc/conv_blk_dec.hip,
    blk_dec.hip) -- needs bf16 cells, whole 8-channel cells at every level and the 8-channel conv_out (hidden_size % 128 == 0)"""
    if not BLK_ENABLED[0]:
        return False
    hs = [c.hidden_size for c in decoder.clstm_list]
    if not all(getattr(c, "dtype", ops.DTYPE_F32) == ops.DTYPE_BF16 for c in decoder.clstm_list):
        return False
    if any(h % 8 for h in hs) or any(_chan(f) % 8 for f in skip_feats) or hs[-1] != 8:
        return False
    return (2 * skip_feats[-1].shape[3]) % 4 == 0


class _Level(object):
    """mode: how the level's input meets its skip feature ("concat" at level 0, decoder.skip_mode above).  hoist / G are None where the
    mode has no time-invariant gate term (mul, none): the gate launches then take the bias instead of the addend.  skip: the feature in the
    layout's storage (None under none); UP[t]: up(h[i-1][t]), under mul the product up(h[i-1][t]) * skip"""
    __slots__ = ("cell", "mode", "hid", "c_up", "c_skip", "H", "W", "hoist", "dyn", "fwd_pack", "G", "Hs", "Cs", "ACT", "UP", "KEY", "SIDE", "ARG", "skip")


UPCONV = [os.environ.get("RSIS_UPCONV", "1") != "0"]       # the last level's upsample + conv_out as one op per direction (upconv_out.hip)


def _heads_bwd_all_steps(L, levels, hs, n, T, B, Wc, Ws, probs_tb, dp_tb, ds_tb, dsides, hb):
    """backward of the class / stop heads: the T * B rows of all timesteps in ONE launch (every row is independent; the parameter
    gradients are sums over rows, which the kernel reduces itself) -- per timestep when the rows do not fit the kernel's LDS, and on
    the wide kernels (one launch pair over all T * B rows) where the kernel takes neither: the order of ops.heads_family"""
    def call(rows, sl, wide=False):
        return ops.heads_bwd_launch(L, [lv.SIDE[sl] for lv in levels], hs, rows, Wc, Ws, probs_tb[sl], dp_tb[sl] if dp_tb is not None else None,
                                    ds_tb[sl] if ds_tb is not None else None, [ds[sl] for ds in dsides], hb, wide)
    K, ncls = sum(hs), Wc.shape[0]
    if ops.heads_family(T * B, K, ncls, backward=True) == "small":
        check(call(T * B, slice(None)), "rsis_heads_bwd(all steps)")
    elif ops.heads_family(B, K, ncls, backward=True) == "small":      # more rows than the kernel's LDS holds
        for t in range(T):
            check(call(B, t), "rsis_heads_bwd")
    else:
        check(call(T * B, slice(None), True), "rsis_heads_wide_bwd(all steps)")


class _Side(object):
    """stands in for a level where only its pooled features are read (_heads_bwd_all_steps on the masked copies)"""
    __slots__ = ("SIDE",)

    def __init__(self, side):
        self.SIDE = side


class _Drop(object):
    """the dropout scales of one sequence (rsis_amd.dropout: one generator launch) and the masked head features.  S2 / MC / MS and SIDEC /
    SIDES are flat [T * B * sum(hid)] buffers in the layout of SIDE; s2 = the per-level views of S2, None at -dropout 0 (then no launch
    of the recurrence differs from the ones made without dropout: only the heads see masks)"""
    __slots__ = ("S2", "MC", "MS", "s2", "SIDEC", "SIDES")


def _heads_fwd_masked(L, SIDE, drop, hs, T, B, Wc, bc, Ws, bs, probs_tb, stop_tb):
    """the heads under dropout, on the decoded features SIDE (flat, all levels): SIDE <- s2 * SIDE, then the class head on mc * SIDE and
    the stop head on ms * SIDE (model.py:169-179) -- the existing heads launch once per masked copy (a few us each; the half of each
    launch that the other one owns goes to scratch), composed with one masking kernel"""
    check(L.rsis_dropout_heads_mask(ptr(SIDE), ptr(drop.S2), ptr(drop.MC), ptr(drop.MS), ptr(drop.SIDEC), ptr(drop.SIDES), SIDE.numel(), stream()),
          "rsis_dropout_heads_mask")
    ops.heads_fwd_launch(L, _per_level(drop.SIDEC, hs, T, B), hs, T * B, Wc, bc, Ws, bs, probs_tb, torch.empty_like(stop_tb))
    ops.heads_fwd_launch(L, _per_level(drop.SIDES, hs, T, B), hs, T * B, Wc, bc, Ws, bs, torch.empty_like(probs_tb), stop_tb)


def _heads_bwd_masked(L, drop, hs, T, B, Wc, Ws, probs_tb, dp_tb, ds_tb, DSIDE, hb):
    """backward of _heads_fwd_masked into DSIDE (flat) = d(s2 * decode(KEY)): one heads backward per masked copy (dstop == NULL on the
    class copy, dprobs == NULL on the stop copy), so dWc / dWs are taken against the masked features; then dside = mc * d(class copy) +
    ms * d(stop copy).  hb: the targets of dWc, dbc, dWs, dbs (None: not wanted)"""
    n = len(hs)
    dsc = dss = None
    if dp_tb is not None:
        dsc = torch.empty_like(DSIDE)
        _heads_bwd_all_steps(L, [_Side(v) for v in _per_level(drop.SIDEC, hs, T, B)], hs, n, T, B, Wc, Ws, probs_tb, dp_tb, None,
                             _per_level(dsc, hs, T, B), [hb[0], hb[1], None, None])
    if ds_tb is not None:
        dss = torch.empty_like(DSIDE)
        _heads_bwd_all_steps(L, [_Side(v) for v in _per_level(drop.SIDES, hs, T, B)], hs, n, T, B, Wc, Ws, probs_tb, None, ds_tb,
                             _per_level(dss, hs, T, B), [None, None, hb[2], hb[3]])
    check(L.rsis_dropout_heads_mask_bwd(ptr(dsc), ptr(dss), ptr(drop.MC), ptr(drop.MS), ptr(DSIDE), DSIDE.numel(), stream()),
          "rsis_dropout_heads_mask_bwd")


def _per_level(buf, hs, T, B):
    """views [T][B][hid] of one flat buffer, level after level"""
    return [v.view(T, B, h) for v, h in zip(buf.split([T * B * h for h in hs]), hs)]


def _diagonal(d, n, T):
    """the cells (level i, step t) with i + t == d: independent of each other in either direction"""
    return [(i, d - i) for i in range(n) if 0 <= d - i < T]


def _gate_srcs(lv, t):
    """the sources of cell (lv, t)'s gate conv besides the hoisted skip term, in packing order: up(h[i-1][t]), h[i][t-1]"""
    return ([lv.UP[t]] if lv.c_up > 0 else []) + ([lv.Hs[t - 1]] if t > 0 else [])


class _Layout(object):
    """How the node stores the recurrence and which kernels it launches on it.  The node asks a layout for the tensors of that storage
    (`empty`) and for the launches that differ between formats; everything else -- the diagonals, the heads, the fused upconv tail, the
    cell state and its gradient (always fp32 NCHW), the parameter-gradient targets -- is the node's."""

    def __init__(self, L, T, B, dev):
        self.L, self.T, self.B, self.dev = L, T, B, dev


class _Nchw(_Layout):
    """fp32 NCHW storage: -dtype fp32, and -dtype bf16 under RSIS_DECODER_BLK=0 (bf16 operands, the round-3 path).  The hoisted skip
    terms, the inter-level upsamples and their transposes and the skip data gradients go out one launch per cell or level."""
    blk = 0                 # the storage flag of rsis_upconv_out_*
    by_level = True         # the per-level tail of the backward runs one level at a time

    def empty(self, lead, C, H, W):
        return torch.empty(lead + (C, H, W), dtype=torch.float32, device=self.dev)

    def to_nchw(self, x):
        return x
    from_nchw = to_nchw

    def hoist(self, levels, feats, gates_w, gates_b, need_grad):
        """G_i = W[:, skip channels] * skip_i + b, one launch per level (on a tile of its own when a backward may follow)"""
        _lib.require_cuda_f32(*feats)
        for lv, f, w, b in zip(levels, feats, gates_w, gates_b):
            lv.skip = f if lv.mode != "none" else None
            if lv.hoist is None:
                continue
            wp = lv.hoist.fwd(w, b)
            check(self.L.rsis_conv2d_fwd(ptr_array([f]), int_array([lv.c_skip]), 1, self.B, lv.H, lv.W, ptr(wp), 4 * lv.hid, 3, 1, 1,
                                         ptr(lv.hoist.bias_p), None, ptr(lv.G), lv.H, lv.W, ops.FORCE_TILE[0] + (100 if need_grad else 0),
                                         lv.hoist.dtype, stream()), "rsis_conv2d_fwd(hoist)")

    def gates(self, levels, cells, wps):
        jobs = (_lib.LstmJob * len(cells))()
        for j, (i, t) in zip(jobs, cells):
            lv = levels[i]
            srcs = _gate_srcs(lv, t)
            j.nsrc = len(srcs)
            for k, s in enumerate(srcs):
                j.src[k], j.Csrc[k] = s.data_ptr(), s.shape[1]
            (j.B, j.H, j.W, j.Wp, j.bias_packed, j.addend, j.c_prev, j.h_out, j.c_out, j.act_out, j.hid, j.ks, j.pad, j.tile, j.dtype,
             j.side_key) = (self.B, lv.H, lv.W, wps[i].data_ptr(), lv.fwd_pack.bias_p.data_ptr() if lv.G is None else None,
                            lv.G.data_ptr() if lv.G is not None else None, lv.Cs[t - 1].data_ptr() if t > 0 else None,
                            lv.Hs[t].data_ptr(), lv.Cs[t].data_ptr(), lv.ACT[t].data_ptr() if lv.ACT is not None else None, lv.hid, 3, 1,
                            ops.FORCE_TILE[0], lv.fwd_pack.dtype, lv.KEY[t].data_ptr())
        check(self.L.rsis_convlstm_fwd_batch(jobs, len(cells), stream()), "rsis_convlstm_fwd_batch")

    def up(self, levels, cells, s2=None):
        """UP[i + 1][t] = up(h[i][t]); s2 (per level [T][B][hid], the Dropout2d scales): s2 * up(h), model.py:141,149-150"""
        for i, t in cells:
            if i + 1 < len(levels):
                lv, nx = levels[i], levels[i + 1]
                if nx.mode == "mul":                      # up(h) * skip (equal sizes: the product itself)
                    check(self.L.rsis_upsample_bilinear_ac_mul_fwd(ptr(lv.Hs[t]), ptr(nx.skip), ptr(nx.UP[t]), self.B * lv.hid, lv.H, lv.W, nx.H, nx.W,
                                                                   stream()), "rsis_upsample_mul_fwd")
                elif s2 is not None:                      # (equal sizes: the scaled copy)
                    check(self.L.rsis_upsample_bilinear_ac_scaled_fwd(ptr(lv.Hs[t]), ptr(s2[i][t]), ptr(nx.UP[t]), self.B * lv.hid, lv.H, lv.W, nx.H,
                                                                      nx.W, stream()), "rsis_upsample_scaled_fwd")
                elif (nx.H, nx.W) == (lv.H, lv.W):        # align-corners resize to the same size is the identity (ops.upsample_bilinear_ac)
                    nx.UP[t].copy_(lv.Hs[t])
                else:
                    check(self.L.rsis_upsample_bilinear_ac_fwd(ptr(lv.Hs[t]), ptr(nx.UP[t]), self.B * lv.hid, lv.H, lv.W, nx.H, nx.W, stream()),
                          "rsis_upsample_fwd")

    def tail(self, last, UP5, conv_out, co_w, co_b, out_masks, heads, sc=None):
        """the x2 upsample of the last level over all steps (times its Dropout2d scales sc [T][B][hid], if any), heads() (the launch of
        the class / stop heads, which each layout issues where it always has), then conv_out: stacked over T where rsis_conv_out_seq_*
        covers the shape (3 launches instead of 3 T), per step otherwise"""
        L, T, B = self.L, self.T, self.B
        H5, W5 = 2 * last.H, 2 * last.W
        if sc is not None:
            check(L.rsis_upsample_bilinear_ac_scaled_fwd(ptr(last.Hs), ptr(sc), ptr(UP5), T * B * last.hid, last.H, last.W, H5, W5, stream()),
                  "rsis_upsample_scaled_fwd(all steps)")
        else:
            check(L.rsis_upsample_bilinear_ac_fwd(ptr(last.Hs), ptr(UP5), T * B * last.hid, last.H, last.W, H5, W5, stream()), "rsis_upsample_fwd(all steps)")
        heads()
        co_pack = conv_out._pack
        co_wp = co_pack.fwd(co_w)
        self.seq_ok = last.hid in (4, 8, 16) and W5 % 4 == 0
        if self.seq_ok:
            check(L.rsis_conv_out_seq_fwd(ptr(UP5), ptr(co_wp), ptr(co_b.detach()), ptr(out_masks), T, B, last.hid, H5, W5, stream()),
                  "rsis_conv_out_seq_fwd")
        else:
            tmp = torch.empty((B, 1, H5, W5), dtype=torch.float32, device=self.dev)
            for t in range(T):
                check(L.rsis_conv2d_fwd(ptr_array([UP5[t]]), int_array([last.hid]), 1, B, H5, W5, ptr(co_wp), 1, 3, 1, 1, ptr(co_b.detach()), None,
                                        ptr(tmp), H5, W5, ops.FORCE_TILE[0], co_pack.dtype, stream()), "rsis_conv2d_fwd(conv_out)")
                out_masks[:, t].copy_(tmp.view(B, -1))

    def tail_bwd(self, d_masks, last, UP5, dUP5, conv_out, co_w, dW, db):
        """conv_out's data gradient into dUP5; its weight / bias gradients into the buffers dW() / db() return (None: not wanted)"""
        L, T, B = self.L, self.T, self.B
        H5, W5 = 2 * last.H, 2 * last.W
        co_pack = conv_out._pack
        co_wd = co_pack.dgrad(co_w)
        dW = dW() if dW else None
        db = db() if db else None
        if self.seq_ok:
            check(L.rsis_conv_out_seq_dgrad(ptr(d_masks), ptr(co_wd), ptr(dUP5), T, B, last.hid, H5, W5, stream()), "rsis_conv_out_seq_dgrad")
            if dW is not None:
                check(L.rsis_conv_out_seq_wgrad(ptr(d_masks), ptr(UP5), ptr(dW), ptr(db), T, B, last.hid, H5, W5, stream()), "rsis_conv_out_seq_wgrad")
            elif db is not None:
                db += d_masks.sum()
            return
        for t in range(T):
            dy = d_masks[:, t].contiguous().view(B, 1, H5, W5)
            check(L.rsis_conv2d_dgrad(ptr(dy), B, 1, H5, W5, ptr(co_wd), co_pack.cin, 3, 1, 1, ptr_array([dUP5[t]]), int_array([last.hid]), 1,
                                      H5, W5, None, ops.FORCE_TILE[0], co_pack.dtype, stream()), "rsis_conv2d_dgrad(conv_out)")
            if dW is not None:
                check(L.rsis_conv2d_wgrad(ptr(dy), ptr(UP5[t]), ptr(dW), B, last.hid, H5, W5, 1, H5, W5, 3, 1, 1, last.hid, 0, 0, co_pack.dtype,
                                          stream()), "rsis_conv2d_wgrad(conv_out)")
            if db is not None:
                check(L.rsis_bias_grad(ptr(dy), ptr(db), B, 1, H5 * W5, 0, stream()), "rsis_bias_grad(conv_out)")

    def up5_bwd(self, dUP5, dside, last, DH_last, sc=None):
        if sc is not None:
            check(self.L.rsis_upsample_maxpool_scaled_bwd(ptr(dUP5), ptr(dside), ptr(last.ARG), ptr(sc), ptr(DH_last), self.T * self.B * last.hid,
                                                          last.H, last.W, 2 * last.H, 2 * last.W, stream()), "rsis_upsample_maxpool_scaled_bwd(all steps)")
            return
        check(self.L.rsis_upsample_maxpool_bwd(ptr(dUP5), ptr(dside), ptr(last.ARG), ptr(DH_last), self.T * self.B * last.hid, last.H, last.W,
                                               2 * last.H, 2 * last.W, stream()), "rsis_upsample_maxpool_bwd(all steps)")

    def up_bwd(self, levels, cells, DUP, DH, dsides, s2=None, DM=None):
        """dh[i][t] = up^T(dUP[i + 1][t]) + the side gradient at the arg-max; s2: times the Dropout2d scale of the plane.  mul levels
        first: DM[i + 1] (+)= dUP * up(h[i][t]) (stored at t = T - 1, the first step the reverse wavefront visits), dUP <- dUP * skip"""
        B = self.B
        for i, t in cells:
            if i + 1 < len(levels):
                lv, nx = levels[i], levels[i + 1]
                if nx.mode == "mul":
                    check(self.L.rsis_upsample_mul_bwd_prep(ptr(DUP[i + 1]), ptr(lv.Hs[t]), ptr(nx.skip), ptr(DM[i + 1]), B * lv.hid, lv.H, lv.W, nx.H,
                                                            nx.W, int(t != self.T - 1), stream()), "rsis_upsample_mul_bwd_prep")
                if s2 is not None and (nx.H, nx.W) == (lv.H, lv.W):
                    check(self.L.rsis_scale_planes(ptr(DUP[i + 1]), ptr(s2[i][t]), ptr(DH[i]), B * lv.hid, lv.H * lv.W, stream()), "rsis_scale_planes")
                    check(self.L.rsis_global_maxpool_scaled_bwd_add(ptr(dsides[i][t]), ptr(lv.ARG[t]), ptr(s2[i][t]), ptr(DH[i]), B * lv.hid,
                                                                    lv.H * lv.W, stream()), "rsis_global_maxpool_scaled_bwd_add")
                elif s2 is not None:
                    check(self.L.rsis_upsample_maxpool_scaled_bwd(ptr(DUP[i + 1]), ptr(dsides[i][t]), ptr(lv.ARG[t]), ptr(s2[i][t]), ptr(DH[i]),
                                                                  B * lv.hid, lv.H, lv.W, nx.H, nx.W, stream()), "rsis_upsample_maxpool_scaled_bwd")
                elif (nx.H, nx.W) == (lv.H, lv.W):
                    DH[i].copy_(DUP[i + 1])
                    check(self.L.rsis_global_maxpool_bwd_add(ptr(dsides[i][t]), ptr(lv.ARG[t]), ptr(DH[i]), B * lv.hid, lv.H * lv.W, stream()),
                          "rsis_global_maxpool_bwd_add")
                else:
                    check(self.L.rsis_upsample_maxpool_bwd(ptr(DUP[i + 1]), ptr(dsides[i][t]), ptr(lv.ARG[t]), ptr(DH[i]), B * lv.hid, lv.H, lv.W,
                                                           nx.H, nx.W, stream()), "rsis_upsample_maxpool_bwd")

    def lstm_bwd(self, jobs):
        """the pointwise LSTM backward of one diagonal, jobs (dh, dh2, dc_next, act, c_prev, c, da, dc_prev): one grouped launch"""
        lb = (_lib.LstmBwdJob * len(jobs))()
        for j, job in zip(lb, jobs):
            j.dh, j.dh2, j.dc_next, j.act, j.c_prev, j.c, j.da, j.dc_prev = [ptr(x) for x in job]
            dh = job[0]
            j.B, j.hid, j.HW = dh.shape[0], dh.shape[1], dh.shape[2] * dh.shape[3]
        check(self.L.rsis_convlstm_bwd_gates_batch(lb, len(jobs), stream()), "rsis_convlstm_bwd_gates_batch")

    def dgrad(self, jobs):
        """the gate convs' data gradients of one diagonal, jobs (dy, packed weights, packed input channels, dtype, [dx, ...]): one
        grouped launch"""
        if not jobs:
            return
        dg = (_lib.DgradJob * len(jobs))()
        for j, (dy, wd, cin, dtype, dxs) in zip(dg, jobs):
            B, Cout, H, W = dy.shape
            (j.dy, j.B, j.Cout, j.Hy, j.Wy, j.Wd, j.Cin_packed, j.ks, j.stride, j.pad, j.ndst, j.Hx, j.Wx, j.addend, j.tile, j.dtype) = (
                ptr(dy), B, Cout, H, W, ptr(wd), cin, 3, 1, 1, len(dxs), H, W, None, ops.FORCE_TILE[0], dtype)
            for k, x in enumerate(dxs):
                j.dx[k], j.Cdx[k] = x.data_ptr(), x.shape[1]
        check(self.L.rsis_conv2d_dgrad_batch(dg, len(jobs), stream()), "rsis_conv2d_dgrad_batch")

    def sum_t(self, DA, dG):
        check(self.L.rsis_sum_leading(ptr(DA), ptr(dG), self.T, dG.numel(), stream()), "rsis_sum_leading")

    def skip_dgrad(self, jobs):
        """dgrad() of the hoisted skip terms: one launch per level"""
        for dy, wd, cin, dtype, (dx,) in jobs:
            B, Cout, H, W = dy.shape
            check(self.L.rsis_conv2d_dgrad(ptr(dy), B, Cout, H, W, ptr(wd), cin, 3, 1, 1, ptr_array([dx]), int_array([dx.shape[1]]), 1, H, W, None,
                                           ops.FORCE_TILE[0], dtype, stream()), "rsis_conv2d_dgrad(hoist)")

    def bias_grad(self, dG, db, lv):
        check(self.L.rsis_bias_grad(ptr(dG), ptr(db), self.B, 4 * lv.hid, lv.H * lv.W, lv.hid, stream()), "rsis_bias_grad(hoist)")

    def wgrad_formats(self, lv):
        """(dtype of the skip term's weight gradient, dtype of the recurrent channels' time-batched ones, source [T][B] -> their rows).
        bf16 rows that are not a multiple of 4 pixels (the 7 / 14-pixel levels of a 224 x 224 input) go through channel-blocked bf16
        copies of the (small) stacks and the whole-cell loader, see decoder_fused._StepFn.backward"""
        if lv.dyn.dtype == ops.DTYPE_BF16 and decoder_fused._BLK_WGRAD[0] and lv.W % 4 != 0 and lv.hid % 8 == 0 and lv.c_up % 8 == 0:
            return lv.dyn.dtype, ops.DTYPE_BF16_BLK, lambda x: ops.blk_from_nchw(x.flatten(0, 1))
        return lv.dyn.dtype, lv.dyn.dtype, lambda x: x.flatten(0, 1)


class _Blk(_Layout):
    """channel-blocked bf16 storage [B][C/8][H][W][8] (csrc/conv_blk_dec.hip, blk_dec.hip) of hidden states, saved gates, up-sampled
    inputs, the hoisted gate terms and every gradient of them.  Per diagonal ONE grouped launch per kind of work (gate convs, upsamples;
    backward: upsample transposes, pointwise LSTM backward, data gradients); the hoisted skip terms and their data gradients of all
    levels in one launch each."""
    blk = 1
    by_level = False        # the per-level tail of the backward runs each of its steps over all levels

    def empty(self, lead, C, H, W):
        return torch.empty(lead + (C // 8, H, W, 8), dtype=torch.bfloat16, device=self.dev)

    def to_nchw(self, x):
        return ops.blk_to_nchw(x)

    def from_nchw(self, x):
        return ops.blk_from_nchw(x)

    def hoist(self, levels, feats, gates_w, gates_b, need_grad):
        jobs = []
        for lv, f, w, b in zip(levels, feats, gates_w, gates_b):
            lv.skip = None if lv.mode == "none" else (f if _is_blk(f) else ops.blk_from_nchw(f))
            if lv.hoist is None:
                continue
            jobs.append(ops.blk_conv_job([lv.skip], lv.hoist.fwd(w, b), 4 * lv.hid, bias=lv.hoist.bias_p, dsts=[lv.G]))
        ops.blk_conv3x3_batch(jobs)

    def gates(self, levels, cells, wps):
        jobs = []
        for i, t in cells:
            lv = levels[i]
            jobs.append(ops.blk_conv_job(_gate_srcs(lv, t), wps[i], 4 * lv.hid, bias=lv.fwd_pack.bias_p if lv.G is None else None, addend=lv.G,
                                         hid=lv.hid, c_prev=lv.Cs[t - 1] if t > 0 else None, c_out=lv.Cs[t], h_out=lv.Hs[t],
                                         act_out=lv.ACT[t] if lv.ACT is not None else None, side_key=lv.KEY[t], shape=(self.B, lv.H, lv.W)))
        ops.blk_conv3x3_batch(jobs)

    def up(self, levels, cells, s2=None):
        cells = [(i, t) for i, t in cells if i + 1 < len(levels)]
        muls = [ops.blk_resize_mul_job(levels[i].Hs[t], levels[i + 1].UP[t], levels[i + 1].skip) for i, t in cells if levels[i + 1].mode == "mul"]
        if muls:            # (every level above 0 has the decoder's mode: a diagonal's upsamples are all of one kind)
            ops.blk_upsample_mul_fwd_batch(muls)
            return
        ups = [ops.blk_resize_job(levels[i].Hs[t], levels[i + 1].UP[t], scale=s2[i][t] if s2 is not None else None) for i, t in cells]
        if ups:
            ops.blk_upsample_fwd_batch(ups)

    def tail(self, last, UP5, conv_out, co_w, co_b, out_masks, heads, sc=None):
        """heads(), then the x2 upsample of the last level (times its Dropout2d scales sc, if any) and conv_out, each over all steps at once"""
        heads()
        ops.blk_upsample_fwd_batch([ops.blk_resize_job(last.Hs.flatten(0, 1), UP5.flatten(0, 1), scale=sc)])
        check(self.L.rsis_blk_conv_out_seq_fwd(ptr(UP5), ptr(co_w.detach()), ptr(co_b.detach()), ptr(out_masks), self.T, self.B, 2 * last.H,
                                               2 * last.W, stream()), "rsis_blk_conv_out_seq_fwd")

    def tail_bwd(self, d_masks, last, UP5, dUP5, conv_out, co_w, dW, db):
        L, T, B = self.L, self.T, self.B
        H5, W5 = 2 * last.H, 2 * last.W
        check(L.rsis_blk_conv_out_seq_dgrad(ptr(d_masks), ptr(co_w.detach()), ptr(dUP5), T, B, H5, W5, stream()), "rsis_blk_conv_out_seq_dgrad")
        if dW or db:
            dW = dW() if dW else torch.zeros_like(co_w)
            db = db() if db else None
            check(L.rsis_blk_conv_out_seq_wgrad(ptr(d_masks), ptr(UP5), ptr(dW), ptr(db), T, B, H5, W5, stream()), "rsis_blk_conv_out_seq_wgrad")

    def up5_bwd(self, dUP5, dside, last, DH_last, sc=None):
        ops.blk_upsample_bwd_batch([ops.blk_resize_job(dUP5.flatten(0, 1), DH_last.flatten(0, 1), dside, last.ARG, backward=True, scale=sc)])

    def up_bwd(self, levels, cells, DUP, DH, dsides, s2=None, DM=None):
        prep = [ops.blk_mul_prep_job(DUP[i + 1], levels[i].Hs[t], levels[i + 1].skip, DM[i + 1], t != self.T - 1)
                for i, t in cells if i + 1 < len(levels) and levels[i + 1].mode == "mul"]
        if prep:
            ops.blk_upsample_mul_bwd_prep_batch(prep)
        ups = [ops.blk_resize_job(DUP[i + 1], DH[i], dsides[i][t], levels[i].ARG[t], backward=True, scale=s2[i][t] if s2 is not None else None)
               for i, t in cells if i + 1 < len(levels)]
        if ups:
            ops.blk_upsample_bwd_batch(ups)

    def lstm_bwd(self, jobs):
        ops.blk_lstm_bwd_batch([ops.blk_lstm_bwd_job(*job) for job in jobs])

    def dgrad(self, jobs):
        if jobs:
            ops.blk_conv3x3_batch([ops.blk_conv_job([dy], wd, sum(x.shape[1] for x in dxs) * 8, cpack=cin, dsts=dxs) for dy, wd, cin, _dt, dxs in jobs])

    def sum_t(self, DA, dG):
        check(self.L.rsis_blk_sum_leading(ptr(DA), ptr(dG), self.T, dG.numel() // 8, stream()), "rsis_blk_sum_leading")

    skip_dgrad = dgrad      # (the skip data gradients of all levels: one grouped launch)

    def bias_grad(self, dG, db, lv):
        check(self.L.rsis_blk_bias_grad(ptr(dG), ptr(db), self.B, 4 * lv.hid, lv.H * lv.W, lv.hid, stream()), "rsis_blk_bias_grad")

    def wgrad_formats(self, lv):
        return ops.DTYPE_BF16_BLK, ops.DTYPE_BF16_BLK, lambda x: x.flatten(0, 1)


class _DecoderSeqFn(torch.autograd.Function):
    """the schedule of the module docstring, on the storage of `layout` (_Nchw or _Blk)"""

    @staticmethod
    def forward(ctx, layout, decoder, T, keep, want_hidden, *tensors):
        L = lib()
        n = len(decoder.clstm_list)
        feats = [t.contiguous() for t in tensors[:n]]      # fp32 NCHW, or already blk (the encoder's blk skip path)
        params = tensors[n:]
        gates_w, gates_b = params[0:2 * n:2], params[1:2 * n:2]
        co_w, co_b, Wc, bc, Ws, bs = params[2 * n:2 * n + 6]
        _lib.require_cuda_f32(*params)
        need_grad = bool(keep) and any(ctx.needs_input_grad)     # (grad mode is off inside forward: the caller says whether a backward may follow)
        dev = feats[0].device
        B = feats[0].shape[0]
        lay = layout(L, T, B, dev)
        hs = [c.hidden_size for c in decoder.clstm_list]
        tot = sum(hs)
        f32 = dict(dtype=torch.float32, device=dev)
        # one zeroed key buffer for the side max-pools of the whole sequence (rsis_lstm_job.side_key), decoded by the heads launch
        KEY = torch.zeros(T * B * tot, dtype=torch.int64, device=dev)
        SIDE = torch.empty(T * B * tot, **f32)
        ARG = torch.empty(T * B * tot, dtype=torch.int32, device=dev)
        levels = []
        for i, cell in enumerate(decoder.clstm_list):
            lv = _Level()
            lv.cell, lv.hid, lv.c_up, lv.c_skip = cell, hs[i], (0 if i == 0 else hs[i - 1]), _chan(feats[i])
            lv.mode = "concat" if i == 0 else decoder.skip_mode
            lv.H, lv.W = feats[i].shape[2], feats[i].shape[3]
            lv.hoist, lv.dyn = decoder_fused._packs(cell, lv.c_up, lv.c_skip, lv.mode)
            lv.G = lay.empty((B,), 4 * lv.hid, lv.H, lv.W) if lv.hoist is not None else None
            lv.Hs = lay.empty((T, B), lv.hid, lv.H, lv.W)
            lv.Cs = torch.empty((T, B, lv.hid, lv.H, lv.W), **f32)
            lv.ACT = lay.empty((T, B), 4 * lv.hid, lv.H, lv.W) if need_grad else None
            lv.UP = lay.empty((T, B), lv.c_up, lv.H, lv.W) if lv.c_up > 0 else None
            levels.append(lv)
        for lv, key, side, arg in zip(levels, _per_level(KEY, hs, T, B), _per_level(SIDE, hs, T, B), _per_level(ARG, hs, T, B)):
            lv.KEY, lv.SIDE, lv.ARG = key, side, arg
        # G_i = W[:, skip channels] * skip_i + b, once per iteration (the skip features do not depend on t); mul / none: no such term
        # the dropout scales of the whole sequence (model.py:141,172,177), drawn once; all rates 0: nothing is allocated or drawn
        drop = None
        p2, pc, ps = dropout.rates(decoder)
        if p2 > 0 or pc > 0 or ps > 0:
            drop = _Drop()
            drop.S2, drop.MC, drop.MS = dropout.draw(dropout.decoder_state(decoder, dev), T * B * tot, p2, pc, ps)
            drop.s2 = _per_level(drop.S2, hs, T, B) if p2 > 0 else None
            drop.SIDEC, drop.SIDES = torch.empty(T * B * tot, **f32), torch.empty(T * B * tot, **f32)
        s2 = drop.s2 if drop is not None else None
        lay.hoist(levels, feats, gates_w, gates_b, need_grad)
        last = levels[-1]
        H5, W5 = 2 * last.H, 2 * last.W
        # (-dropout > 0: the last level goes through the unfused tail, whose upsample takes the scale)
        upc = UPCONV[0] and s2 is None and L.rsis_upconv_out_supported(last.hid, last.H, last.W, H5, W5) == 1
        UP5 = None if upc else lay.empty((T, B), last.hid, H5, W5)            # model.py:163-164, all timesteps
        probs_tb = torch.empty((T, B, Wc.shape[0]), **f32)
        stop_tb = torch.empty((T, B, 1), **f32)
        for i, lv in enumerate(levels):          # (the limb copy where the routing puts the level's training forward on the limb kernel)
            lv.fwd_pack = decoder_fused.dyn_fwd_pack(lv.cell, lv.c_up, lv.c_skip, i, need_grad and not lay.blk, lv.mode)
        # (a level without a hoisted term gets its bias from the gate launch: packed with the copy that launch reads)
        wps = [lv.fwd_pack.fwd(w) if lv.hoist is not None else lv.fwd_pack.fwd(w, b) for lv, w, b in zip(levels, gates_w, gates_b)]
        for d in range(T + n - 1):
            cells = _diagonal(d, n, T)
            lay.gates(levels, cells, wps)
            if s2 is not None:
                lay.up(levels, cells, s2)
            else:
                lay.up(levels, cells)
            # (the x2 upsample of the last level, model.py:163-164, feeds conv_out only, and the heads only the losses: both run once
            #  over all T steps after the loop)

        def heads():
            """the class / stop heads (model.py:169-182) of ALL timesteps in one launch: every (t, b) row is independent, the per-level
            key / feature / arg-max arrays are [T][B][hid] contiguous, i.e. T * B rows; the launch decodes the pooled keys (writes SIDE / ARG)"""
            ops.heads_fwd_launch(L, [v.SIDE for v in levels], hs, T * B, Wc, bc, Ws, bs, probs_tb, stop_tb,
                                 ([v.KEY for v in levels], [v.ARG for v in levels]))
            if drop is not None:
                _heads_fwd_masked(L, SIDE, drop, hs, T, B, Wc, bc, Ws, bs, probs_tb, stop_tb)
        # conv_out (model.py:167) on every timestep at once, logits straight into (B, T, N)
        out_masks = torch.empty((B, T, H5 * W5), **f32)
        if upc:       # upsample + conv_out in one pass, the upsampled tensor never formed (nor rounded to bf16)
            heads()
            check(L.rsis_upconv_out_fwd(ptr(last.Hs), lay.blk, ptr(co_w.detach()), ptr(co_b.detach()), ptr(out_masks), T, B, last.hid, last.H, last.W,
                                        H5, W5, stream()), "rsis_upconv_out_fwd")
        else:
            if s2 is not None:
                lay.tail(last, UP5, decoder.conv_out, co_w, co_b, out_masks, heads, s2[n - 1])
            else:
                lay.tail(last, UP5, decoder.conv_out, co_w, co_b, out_masks, heads)
        out_probs = probs_tb.transpose(0, 1).contiguous()            # (B, T, C)   train.py:119
        out_stops = stop_tb.transpose(0, 1).contiguous()             # (B, T, 1)   train.py:120
        hidden = []
        if want_hidden:
            for lv in levels:
                hidden += [lay.to_nchw(lv.Hs[T - 1]), lv.Cs[T - 1]]
        if RECORD[0]:
            LAST["arg"] = [lv.ARG.clone() for lv in levels]
            if drop is not None:
                LAST["drop"] = {"s2": [v.clone() for v in s2] if s2 is not None else None, "mc": [v.clone() for v in _per_level(drop.MC, hs, T, B)],
                                "ms": [v.clone() for v in _per_level(drop.MS, hs, T, B)]}
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.lay, ctx.decoder, ctx.T, ctx.levels, ctx.upc = lay, decoder, T, levels, upc
            ctx.UP5, ctx.probs_tb, ctx.feats, ctx.params = UP5, probs_tb, feats, params
            ctx.drop = drop
        else:
            for lv in levels:
                lv.G = lv.ACT = lv.UP = lv.skip = None
        return (out_masks, out_probs, out_stops) + tuple(hidden)

    @staticmethod
    def backward(ctx, d_masks, d_probs, d_stops, *d_hidden):
        L = lib()
        lay, decoder, T, levels = ctx.lay, ctx.decoder, ctx.T, ctx.levels
        n = len(levels)
        feats, params = ctx.feats, ctx.params
        gates_w = params[0:2 * n:2]
        co_w, co_b, Wc, bc, Ws, bs = params[2 * n:2 * n + 6]
        need = ctx.needs_input_grad            # (layout, decoder, T, keep, want_hidden, feats..., params...)
        need_feat = [need[5 + i] for i in range(n)]
        need_par = [need[5 + n + k] for k in range(len(params))]
        dev = feats[0].device
        B = feats[0].shape[0]
        hs = [lv.hid for lv in levels]
        f32 = dict(dtype=torch.float32, device=dev)
        last = levels[-1]
        H5, W5 = 2 * last.H, 2 * last.W
        UP5 = ctx.UP5
        drop = ctx.drop
        s2 = drop.s2 if drop is not None else None
        grads_par = [None] * len(params)

        def target(k):
            """(buffer the kernels accumulate parameter k's gradient into, is it the flat gradient buffer)"""
            p = params[k]
            t = ops._direct_target(p)
            if t is not None:
                return t, True
            g = torch.zeros_like(p)
            grads_par[k] = g
            return g, False

        # ---- conv_out: data gradient of all T steps, weight + bias gradient ----
        upc = ctx.upc
        dUP5 = None if upc else torch.empty_like(UP5)
        kw, kb = 2 * n, 2 * n + 1
        have_masks = d_masks is not None       # (no gradient on the logits: conv_out's parameters get none either, as on the unfused path)
        if upc:         # (the whole tail runs below, once the side gradients of the heads are known)
            d_masks = torch.zeros((B, T, H5 * W5), **f32) if d_masks is None else d_masks.contiguous()
        elif d_masks is None:
            dUP5.zero_()
        else:
            lay.tail_bwd(d_masks.contiguous(), last, UP5, dUP5, decoder.conv_out, co_w, (lambda: target(kw)[0]) if need_par[kw] else None,
                         (lambda: target(kb)[0]) if need_par[kb] else None)
        # ---- heads: all timesteps (the parameter gradients accumulate over t) ----
        DSIDE = torch.empty(T * B * sum(hs), **f32)
        dsides = _per_level(DSIDE, hs, T, B)
        if d_probs is None and d_stops is None:
            DSIDE.zero_()
        else:
            dp_tb = d_probs.transpose(0, 1).contiguous() if d_probs is not None else None
            ds_tb = d_stops.transpose(0, 1).contiguous() if d_stops is not None else None
            hb = [target(2 * n + 2 + k)[0] if need_par[2 * n + 2 + k] else None for k in range(4)]
            if drop is None:
                _heads_bwd_all_steps(L, levels, hs, n, T, B, Wc, Ws, ctx.probs_tb, dp_tb, ds_tb, dsides, hb)
            else:
                _heads_bwd_masked(L, drop, hs, T, B, Wc, Ws, ctx.probs_tb, dp_tb, ds_tb, DSIDE, hb)
        # ---- reverse wavefront ----
        DA = [torch.empty_like(lv.ACT) for lv in levels]
        DH = [lay.empty((B,), lv.hid, lv.H, lv.W) for lv in levels]                  # gradient of h[i][t] from above (upsample + pool)
        DHP = [lay.empty((B,), lv.hid, lv.H, lv.W) for lv in levels]                 # ... through the recurrence, from step t + 1
        DC = [[torch.empty((B, lv.hid, lv.H, lv.W), **f32) for _ in range(2)] for lv in levels]
        DUP = [lay.empty((B,), lv.c_up, lv.H, lv.W) if lv.c_up > 0 else None for lv in levels]
        dpk = [decoder_fused.dyn_dgrad_pack(lv.cell, lv.c_up, lv.c_skip, lv.H, lv.W, level=i, mode=lv.mode) for i, lv in enumerate(levels)]
        # mul: the gradient of the skip feature, summed over t in fp32 NCHW whatever the storage (rounded once, at the end)
        DM = [torch.empty((B, lv.c_up, lv.H, lv.W), **f32) if lv.mode == "mul" else None for lv in levels]
        mul = any(m is not None for m in DM)
        wds = [pk.dgrad(w) for pk, w in zip(dpk, gates_w)]
        # gradients a caller put on the returned final state (none in runIter: train.py never reads it)
        d_hidden = d_hidden or (None,) * (2 * n)
        dhf = [lay.from_nchw(g.contiguous()) if g is not None else None for g in d_hidden[0::2]]
        dcf = [g.contiguous() if g is not None else None for g in d_hidden[1::2]]
        # the last level's hidden states receive their gradient from conv_out only (no level above): all T steps in one launch
        DH_last = lay.empty((T, B), last.hid, last.H, last.W)
        if upc:         # through conv_out and the upsample (plus the side max-pool gradient at its arg-max pixel); dW / db accumulate
            dW = target(kw)[0] if need_par[kw] and have_masks else None        # (fixed-order sums of per-block partials)
            db = target(kb)[0] if need_par[kb] and have_masks else None
            partial = torch.empty(L.rsis_upconv_out_bwd_blocks(T, B, last.H, last.W) * 80, **f32)
            check(L.rsis_upconv_out_bwd(ptr(d_masks), ptr(last.Hs), lay.blk, ptr(co_w.detach()), ptr(DH_last), ptr(dW), ptr(db), ptr(dsides[n - 1]),
                                        ptr(last.ARG), ptr(partial), T, B, last.hid, last.H, last.W, H5, W5, stream()), "rsis_upconv_out_bwd")
        else:
            if s2 is not None:
                lay.up5_bwd(dUP5, dsides[n - 1], last, DH_last, s2[n - 1])
            else:
                lay.up5_bwd(dUP5, dsides[n - 1], last, DH_last)
        for d in range(T + n - 2, -1, -1):
            cells = _diagonal(d, n, T)
            # gradient reaching h[i][t] through its upsample into the next level and its side max-pool
            if mul:
                lay.up_bwd(levels, cells, DUP, DH, dsides, None, DM)
            elif s2 is not None:
                lay.up_bwd(levels, cells, DUP, DH, dsides, s2)
            else:
                lay.up_bwd(levels, cells, DUP, DH, dsides)
            lstm, dg = [], []
            for i, t in cells:
                lv = levels[i]
                dh2, dcn = (dhf[i], dcf[i]) if t == T - 1 else (DHP[i], DC[i][(t + 1) & 1])
                lstm.append((DH[i] if i + 1 < n else DH_last[t], dh2, dcn, lv.ACT[t], lv.Cs[t - 1] if t > 0 else None, lv.Cs[t], DA[i][t],
                             DC[i][t & 1] if t > 0 else None))
                dxs = ([DUP[i]] if lv.c_up > 0 else []) + ([DHP[i]] if t > 0 else [])
                if dxs:
                    dg.append((DA[i][t], wds[i], lv.dyn.cin, dpk[i].dtype, dxs))
            # clstm.py:47-58 backwards: d(gates), dc_{t-1} of the diagonal's cells -- ONE grouped launch
            lay.lstm_bwd(lstm)
            # data gradients of the gate convs: d(up[i][t]) for the level below, dh[i][t-1] through the recurrence -- ONE grouped launch
            lay.dgrad(dg)
        # ---- per level, once: the time-invariant skip term and the time-batched weight gradients ----
        # (sum_t d(gates) feeds the hoisted term's data / weight gradient and the bias gradient; without a hoisted term only the latter)
        dG, dskip, dfeats = [None] * n, [None] * n, [None] * n
        hoisted = [lv.hoist is not None for lv in levels]
        for grp in ([[i] for i in range(n)] if lay.by_level else [range(n)]):
            for i in grp:
                if T == 1:
                    dG[i] = DA[i][0]
                elif hoisted[i] or need_par[2 * i + 1]:
                    dG[i] = torch.empty_like(DA[i][0])
                    lay.sum_t(DA[i], dG[i])
                if need_feat[i] and hoisted[i]:
                    dskip[i] = torch.empty_like(levels[i].skip)
            lay.skip_dgrad([(dG[i], levels[i].hoist.dgrad(gates_w[i]), levels[i].hoist.cin, levels[i].hoist.dtype, [dskip[i]]) for i in grp
                            if need_feat[i] and hoisted[i]])
            for i in grp:
                lv = levels[i]
                kw, kb = 2 * i, 2 * i + 1
                hid, H, W = lv.hid, lv.H, lv.W
                if need_feat[i] and hoisted[i]:
                    dfeats[i] = dskip[i] if _is_blk(feats[i]) else lay.to_nchw(dskip[i])
                elif need_feat[i] and lv.mode == "mul":      # (none: the feature is unused, its gradient stays None)
                    dfeats[i] = ops.blk_from_nchw(DM[i]) if _is_blk(feats[i]) else DM[i]
                if need_par[kb]:
                    lay.bias_grad(dG[i], target(kb)[0], lv)
                if need_par[kw]:
                    dW, direct = target(kw)
                    Ctot = gates_w[i].shape[1]
                    dt_skip, dt, rows = lay.wgrad_formats(lv)
                    if hoisted[i]:      # (sum: into columns [0, c_up), which the batched-up launch below adds to)
                        ops.wgrad_launch(L, dG[i], lv.skip, dW, B, lv.c_skip, H, W, 4 * hid, H, W, 3, 1, 1, Ctot, lv.hoist.offs[0], hid, dt_skip,
                                         "rsis_conv2d_wgrad(hoist)", direct)
                    da = rows(DA[i])
                    if lv.c_up > 0:
                        ops.wgrad_launch(L, da, rows(lv.UP), dW, T * B, lv.c_up, H, W, 4 * hid, H, W, 3, 1, 1, Ctot, 0, hid, dt,
                                         "rsis_conv2d_wgrad(batched up)", direct)
                    if T > 1:
                        ops.wgrad_launch(L, da[B:], rows(lv.Hs[:T - 1]), dW, (T - 1) * B, hid, H, W, 4 * hid, H, W, 3, 1, 1, Ctot, lv.dyn.offs[-1],
                                         hid, dt, "rsis_conv2d_wgrad(batched h)", direct)
        for lv in levels:
            lv.G = lv.Hs = lv.Cs = lv.ACT = lv.UP = lv.skip = None
        ctx.lay = ctx.levels = ctx.UP5 = ctx.feats = ctx.params = ctx.decoder = ctx.drop = None
        return (None, None, None, None, None) + tuple(dfeats) + tuple(grads_par)


def decoder_sequence_stacked(decoder, skip_feats, T, want_hidden=True):
    """(out_masks (B, T, H*W) logits, class_probs (B, T, C), stop logits (B, T, 1), hidden_list (None unless want_hidden), (H, W) of the
    masks)"""
    n = len(decoder.clstm_list)
    params = []
    for c in decoder.clstm_list:
        params += [c.Gates.weight, c.Gates.bias]
    params += [decoder.conv_out.weight, decoder.conv_out.bias, decoder.fc_class.weight, decoder.fc_class.bias, decoder.fc_stop.weight,
               decoder.fc_stop.bias]
    keep = torch.is_grad_enabled() and (any(f.requires_grad for f in skip_feats) or any(p.requires_grad for p in params))
    layout = _Blk if blk_supported(decoder, skip_feats) else _Nchw
    res = _DecoderSeqFn.apply(layout, decoder, int(T), keep, bool(want_hidden), *skip_feats, *params)
    out_masks, out_probs, out_stops = res[:3]
    hidden = [[res[3 + 2 * i], res[4 + 2 * i]] for i in range(n)] if len(res) > 3 else None
    size = (2 * skip_feats[-1].shape[2], 2 * skip_feats[-1].shape[3])
    return out_masks, out_probs, out_stops, hidden, size
