"""Case tables and a priori error bounds of test_gpu_heads_wide.py (and of test_heads_wide_host.py, which checks them without a device):
the wide class / stop heads of csrc/losses.hip (rsis_heads_wide_fwd / rsis_heads_wide_bwd).  Input builders and float64 references are
those of loss_path_cases.py; everything here is numpy on the host, nothing imports the library.

EXACT shapes: integers in -3..3 and probs 1 / 2^k (loss_path_cases.heads_exact_data) -- every fp32 operation is exact in any order as
long as every sum of |terms| stays below 2^24 (heads_exact_bound; test_heads_wide_host.py asserts it), so the results must EQUAL float64.

NORMAL shapes: bounds derived here, before any kernel ran.  u = 2^-24 (one fp32 rounding, relative), gamma_n = n u / (1 - n u).

  (a) a sum of n fp32 terms formed in ANY order, the products rounded or fused: every term passes through at most n roundings, so
        |computed - exact| <= gamma_n * sum |terms|                                          (Higham, Accuracy and Stability, 3.1 / 4.2)
      logits (K products + the bias, n = K + 1):  delta[i][r] = gamma_(K+1) * (sum_k |W[r][k] sv[i][k]| + |b[r]|).  The stop logit is
      row ncls of that table: its bound is delta[i][ncls].
  (b) probabilities.  The kernel evaluates softmax on logits l^ = l + eps, |eps_c| <= delta_i = max_c delta[i][c]:
        p~_c / p_c = exp(eps_c) * sum_j exp(l_j) / sum_j exp(l_j + eps_j)  lies in  [exp(-2 delta_i), exp(2 delta_i)],
      so |p~_c - p_c| <= p_c * expm1(2 delta_i).  The fp32 evaluation of softmax(l^) itself: expf within 1 ulp (2 u) on the numerator
      and, weighted, on the terms of the denominator (2 u), the sum of ncls positive terms ((ncls - 1) u in any order), the division
      (u): (ncls + 4) u, relative; the bound allows (ncls + 8) u.  The rounding of l^_c - m (u |l^_c - m| <= 2 u max_c sum |terms|, i.e.
      2 delta_i / (K + 1)) is charged to delta: the kernel's fused chains round a term ceil(K / 64) + 7 times, not the K + 1 times
      gamma_(K+1) pays for.  Hence
        |p^ - p| <= p * (expm1(2 delta_i) + (ncls + 8) u) + TINY,
      TINY = 2^-125: a probability (or its numerator) below the smallest normal fp32, 2^-126, may be flushed to zero -- the float64
      reference of the `hot` regime holds values down to 1e-300 that no fp32 kernel can return.
  (c) backward, from the fp32 inputs (probs, dprobs, dstop) the kernel reads:
        dot_i = sum_c g p (n = ncls):                 E_dot = gamma_ncls * sum_c |g p|
        dl_c = p_c (g_c - dot): one subtraction and one product on a dot that is off by E_dot:
                                                      E_dl = p_c * ((1 + gamma_2) E_dot + gamma_2 |g_c - dot|)
        the stop d-logit is copied: exact.
        d side[i][k] = sum_c dl_c Wc[c][k] + ds Ws[k] (n = ncls + 1), formed from the computed dl^ (|dl^| <= |dl| + E_dl):
                                                      gamma_n * (sum_c (|dl| + E_dl) |Wc| + |ds Ws|) + (1 + gamma_n) sum_c E_dl |Wc|
        dWc[r][k] = sum_i dl[i][r] sv[i][k] (+ the zero the buffer held: n = rows + 1), likewise; dbc[r] with sv = 1;
        dWs[k] = sum_i ds_i sv[i][k] and dbs = sum_i ds_i: exact operands, gamma_(rows+1) * sum |terms|.
      Each backward bound also carries n * 2^-149: an operation whose result falls below 2^-126 rounds to the denormal grid.
No constant here was fitted to what a kernel returns."""
import numpy as np

import loss_path_cases as L

U24 = L.U24
P = [128, 64, 32, 16, 8]
# (rows, Cside, ncls): one row / one feature; odd rows; rows past a chunk of 64 of the parameter pass; the decoder's K = 248 at the COCO
# class count; the first row count the small backward refuses at 21 classes (365) and T * B = 1280; many rows of few classes; K at its limit;
# K and ncls that are no multiple of the 16 x 64 parameter tile, side vectors that straddle a tile
EXACT_SHAPES = [(1, [1], 65), (3, [5], 81), (37, P, 81), (300, P, 81), (365, P, 21), (1280, P, 21), (2600, [16, 8], 9), (9, [2048], 256),
                (17, [300, 7], 256), (130, [7, 300], 100), (20, [2048], 128)]
NORMAL_SHAPES = [(640, P, 81), (70, [2048], 256), (3, [40], 1024)]
BOTH_SHAPE = (64, [2048], 64)          # the small family accepts it too
NULL_SHAPE = (37, P, 81)
TINY = 2.0 ** -125
DENORM = 2.0 ** -149


def gamma(n):
    return n * U24 / (1.0 - n * U24)


def fwd_bounds(d):
    """(bound of probs (rows, ncls), bound of stop (rows,)) for a heads_normal_data case: (a) and (b) above"""
    sv = np.abs(np.concatenate(d["sides"], 1)).astype(np.float64)
    K, ncls = sv.shape[1], d["Wc"].shape[0]
    W_all = np.abs(np.concatenate([d["Wc"], d["Ws"][None, :]], 0)).astype(np.float64)
    b_all = np.abs(np.concatenate([d["bc"], d["bs"]])).astype(np.float64)
    delta = gamma(K + 1) * (sv @ W_all.T + b_all[None, :])
    drow = delta[:, :ncls].max(1, keepdims=True)
    return d["probs"] * (np.expm1(2 * drow) + (ncls + 8) * U24) + TINY, delta[:, ncls]


def bwd_bounds(d, probs=None):
    """{dside (rows, K), dWc, dbc, dWs, dbs} bounds for a case whose backward reads `probs` (default: the case's probs_in): (c) above"""
    p = (d["probs_in"] if probs is None else probs).astype(np.float64)
    g, ds = d["dprobs"].astype(np.float64), np.abs(d["dstop"].astype(np.float64))
    sv = np.abs(np.concatenate(d["sides"], 1)).astype(np.float64)
    aWc, aWs = np.abs(d["Wc"]).astype(np.float64), np.abs(d["Ws"]).astype(np.float64)
    rows, ncls = p.shape
    dot = (g * p).sum(1, keepdims=True)
    e_dot = gamma(ncls) * np.abs(g * p).sum(1, keepdims=True)
    e_dl = p * ((1 + gamma(2)) * e_dot + gamma(2) * np.abs(g - dot))
    adl = np.abs(p * (g - dot)) + e_dl
    n1, n2 = ncls + 1, rows + 1
    return dict(dside=gamma(n1) * (adl @ aWc + ds[:, None] * aWs[None, :]) + (1 + gamma(n1)) * (e_dl @ aWc) + n1 * DENORM,
                dWc=gamma(n2) * (adl.T @ sv) + (1 + gamma(n2)) * (e_dl.T @ sv) + n2 * DENORM,
                dbc=gamma(n2) * adl.sum(0) + (1 + gamma(n2)) * e_dl.sum(0) + n2 * DENORM,
                dWs=gamma(n2) * (ds @ sv) + n2 * DENORM, dbs=np.array([gamma(n2) * ds.sum() + n2 * DENORM]))
