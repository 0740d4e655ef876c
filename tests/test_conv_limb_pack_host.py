"""The packed limb copy of the limb flavour of the direct 3x3 conv (pack.hip: PACK_LIMB_FWD / PACK_LIMB_DGRAD), on the CPU.

The pack kernels themselves run on the GPU: test_gpu_conv_limb.py compares what the library's pack entry points write, byte for byte,
with conv_limb_cases.limb_planes().  This file holds that expectation to its own references, without a GPU:
  * limb_split.h, compiled with the host compiler, must give the limbs conv_limb_cases.split3 computes (the same bits);
  * limb 0 + limb 1 + limb 2 of every packed weight is the weight, bit for bit;
  * read back the way the block program addresses its weight stage (conv_limb_cases.kernel_read: 54 consecutive rows per chunk, limb
    planes of 18, two cells per tap), the copy gives every (row, channel, tap) of the weight at the place the MFMA loop takes it from --
    forward and data gradient (rotated, transposed), gate rows interleaved to 4 j + gate;
  * the size queries and rsis_conv_pack_job_fill of the library (host functions) plan exactly these rows: 1.5 x the bytes of the f32 copy."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import conv_limb_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "limb_split.h"
#include <stdio.h>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  float v[8];
  while (fread(v, 4, 8, f) == 8) {
    unsigned c[3][4];
    rsis_limb_pack8_cells(v, c[0], c[1], c[2]);
    fwrite(c, 4, 12, o);
  }
  fclose(o);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header_cells(tmp_path_factory):
    """runs rsis_limb_pack8_cells of limb_split.h over groups of eight floats; returns f(values [n][8]) -> uint16 [n][3][8]"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("limb_pack")
    (d / "cells.cpp").write_text(SRC)
    exe = str(d / "cells")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rsis_amd", "csrc"), "-o", exe, str(d / "cells.cpp")])

    def run(v):
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 8)
        v.tofile(str(d / "in.bin"))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        return np.fromfile(str(d / "out.bin"), np.uint16).reshape(-1, 3, 8)
    return run


@pytest.mark.parametrize("case", C.PACK_CASES, ids=[c[0] for c in C.PACK_CASES])
def test_numpy_split_is_the_headers(case, header_cells):
    w = C.pack_weight(case)
    flat = w.reshape(-1)[: w.size // 8 * 8]
    cells = header_cells(flat)
    for l, limb in enumerate(C.split3(flat)):
        np.testing.assert_array_equal(cells[:, l].reshape(-1), (limb.view(np.uint32) >> 16).astype(np.uint16))
        assert (limb.view(np.uint32) & 0xFFFF).max() == 0


@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("case", C.PACK_CASES, ids=[c[0] for c in C.PACK_CASES])
def test_planes_are_what_the_kernel_reads(case, dgrad):
    _name, cout, segs, offs, hid = case
    w = C.pack_weight(case)
    planes = C.limb_planes(w, segs, offs, hid, dgrad)
    concat = [o + c for c0, o in zip(segs, offs) for c in range(c0)]
    # the reduction axis as the kernel walks it: (chunk, channel in chunk) -> (weight row, weight input channel) per column, or None
    if not dgrad:
        red, q = [], 0
        for c0, o in zip(segs, offs):
            for qq in range(C.cdiv(c0, C.CKL)):
                red.append([(o + qq * C.CKL + k) if qq * C.CKL + k < c0 else None for k in range(C.CKL)])
        cols = cout
    else:
        red = [[(q * C.CKL + k) if q * C.CKL + k < cout else None for k in range(C.CKL)] for q in range(C.cdiv(cout, C.CKL))]
        cols = len(concat)
    assert planes.shape[0] == 54 * len(red)
    for q, chans in enumerate(red):
        for tap in range(9):
            for col in range(cols):
                v = C.kernel_read(planes, q, tap, col)
                s = (v[0] + v[1]).astype(np.float32) + v[2]                  # exact partial sums: the value itself
                for k, ch in enumerate(chans):
                    if ch is None:
                        assert (v[:, k] == 0).all()
                        continue
                    if not dgrad:
                        want = w[C.ref_row(col, hid), ch, tap // 3, tap % 3]
                    else:
                        want = w[C.ref_row(ch, hid), concat[col], (8 - tap) // 3, (8 - tap) % 3]
                    assert s[k].view(np.uint32) == want.view(np.uint32), (q, tap, col, k)
    # columns past the real ones are zero
    assert not planes[:, cols:].any()


@pytest.mark.parametrize("dgrad", [0, 1], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("case", C.PACK_CASES, ids=[c[0] for c in C.PACK_CASES])
def test_library_plans_these_rows(case, dgrad):
    from rsis_amd import _lib
    L = _lib.lib()
    _name, cout, segs, offs, hid = case
    ctot = max(o + c for c, o in zip(segs, offs))
    rows, ldw = C.plan((cout, ctot, 3, 3), segs, hid, bool(dgrad))
    j = _lib.PackJob()
    j.dgrad, j.dtype, j.Cout, j.Ctot, j.ks, j.stride, j.pad, j.nseg, j.lstm_hid = dgrad, C.F32_LIMB, cout, ctot, 3, 1, 1, len(segs), hid
    for i, (c, o) in enumerate(zip(segs, offs)):
        j.Cseg[i], j.Coff[i] = c, o
    blocks = L.rsis_conv_pack_job_fill(ctypes.byref(j))
    assert blocks > 0 and (j.imode, j.krows, j.ldw) == (10 if dgrad else 9, rows, ldw)
    seg_arr = (ctypes.c_int * len(segs))(*segs)
    if dgrad:
        limb, f32 = (L.rsis_conv_packed_bytes_dgrad(dt, cout, 3, 1, 1, sum(segs)) for dt in (C.F32_LIMB, 0))
    else:
        limb, f32 = (L.rsis_conv_packed_bytes_fwd(dt, cout, 3, 1, 1, len(segs), seg_arr) for dt in (C.F32_LIMB, 0))
    assert limb == rows * ldw * 16
    # 1.5 x the f32 rows wherever the f32 copy's 8-channel chunks pair up into 16-channel ones (a half-empty chunk is padded to a full one)
    pairs = all(c % 16 == 0 for c in ([cout] if dgrad else segs))
    assert (2 * limb == 3 * f32) if pairs else (3 * f32 <= 2 * limb <= 6 * f32)


def test_repack_table_is_keyed_by_the_whole_job():
    """ops.repack_all() rebuilds its job table when anything a job holds changes: two copies at the SAME addresses (a freed PackedConv's id,
    weight and copy addresses can all come back from the allocator) with another dtype, segment list or weight shape have different keys"""
    import torch
    from rsis_amd import ops
    w, out = torch.zeros(40, 24, 3, 3), torch.zeros(16)
    base = ops.PackedConv(3, [24], stride=1, pad=1, dtype=ops.DTYPE_F32_LIMB)
    same = ops.PackedConv(3, [24], stride=1, pad=1, dtype=ops.DTYPE_F32_LIMB)
    assert base._job_sig(w, out, 0) == same._job_sig(w, out, 0) and base._job_sig(w, out, 0) != base._job_sig(w, out, 1)
    others = [ops.PackedConv(3, [24], stride=1, pad=1, dtype=ops.DTYPE_F32), ops.PackedConv(3, [16, 8], stride=1, pad=1, dtype=ops.DTYPE_F32_LIMB),
              ops.PackedConv(3, [16, 8], stride=1, pad=1, offs=[0, 24], dtype=ops.DTYPE_F32_LIMB),
              ops.PackedConv(3, [24], lstm_hid=10, stride=1, pad=1, dtype=ops.DTYPE_F32_LIMB)]
    keys = [base._job_sig(w, out, 0)] + [p._job_sig(w, out, 0) for p in others] + [base._job_sig(w.view(20, 48, 3, 3), out, 0)]
    assert len(set(keys)) == len(keys)
    # every field of the job the library reads is in the key
    j0, j1 = base._job(w, out, 0), others[2]._job(w, out, 0)
    assert bytes(j0) != bytes(j1)


def test_other_geometries_keep_the_f32_plan():
    """under RSIS_DTYPE_F32_LIMB a conv the limb kernel does not cover is planned exactly as under RSIS_DTYPE_F32"""
    from rsis_amd import _lib
    L = _lib.lib()
    for cout, segs, ks, stride, pad in ((40, [20], 3, 1, 1), (40, [24], 3, 2, 1), (40, [24], 1, 1, 0), (1, [8], 3, 1, 1)):
        seg_arr = (ctypes.c_int * len(segs))(*segs)
        assert L.rsis_conv_packed_bytes_fwd(C.F32_LIMB, cout, ks, stride, pad, len(segs), seg_arr) == \
            L.rsis_conv_packed_bytes_fwd(0, cout, ks, stride, pad, len(segs), seg_arr)
    assert L.rsis_conv_packed_bytes_dgrad(C.F32_LIMB, 36, 3, 1, 1, 24) == L.rsis_conv_packed_bytes_dgrad(0, 36, 3, 1, 1, 24)
