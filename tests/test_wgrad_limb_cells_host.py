"""The limb cells of the staged fp32 weight-gradient kernels (rsis_limb_pack8_cells of rsis_amd/csrc/limb_split.h: eight fp32 values ->
three 16-byte cells, one per limb, high halves only, element 2m in the low half of dword m), on the CPU: the header is plain C++ and a
few lines of host code around it are compiled with the system compiler.  For every input the three cells must decode to limbs whose
sum is the input bit for bit -- except below |v| = 2^-103, where the header says the last residual can be a subnormal whose low bits
the pack drops: there the sum is within 2^-126 of the input -- and each decoded limb must equal the high half of the limb
rsis_limb_split3 gives for the same element.  The expected answers are the input itself and rsis_limb_split3."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "limb_split.h"
#include <stdio.h>
#include <string.h>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  float v[8];
  while (fread(v, 4, 8, f) == 8) {
    unsigned c[3][4];
    rsis_limb_pack8_cells(v, c[0], c[1], c[2]);
    fwrite(c, 4, 12, o);                       // the three cells as the kernel stores them
    unsigned ref[8][3];                        // rsis_limb_split3 of every element: the limbs' encodings
    for (int k = 0; k < 8; ++k) {
      float l[3];
      rsis_limb_split3(v[k], l[0], l[1], l[2]);
      memcpy(ref[k], l, 12);
    }
    fwrite(ref, 4, 24, o);
  }
  fclose(o);
  return 0;
}
"""


def _inputs():
    r = np.random.default_rng(20261)
    flt_max = np.finfo(np.float32).max
    parts = [
        r.normal(0, 1, 80000).astype(np.float32),
        (r.normal(0, 1, 40000) * np.exp2(r.integers(-100, 100, 40000))).astype(np.float32),
        r.integers(0, 0x7F800000, 40000, dtype=np.int64).astype(np.uint32).view(np.float32),                    # any finite positive encoding
        (r.integers(0, 0x7F800000, 40000, dtype=np.int64) | 0x80000000).astype(np.uint32).view(np.float32),     # ... negative
        (flt_max * r.uniform(0.5, 1.0, 8000) * r.choice([-1.0, 1.0], 8000)).astype(np.float32),                 # huge
        (r.uniform(0.1, 1.0, 8000) * np.exp2(r.integers(-149, -100, 8000)) * r.choice([-1.0, 1.0], 8000)).astype(np.float32),   # tiny, subnormals included
        r.integers(1, 0x00800000, 8000, dtype=np.int64).astype(np.uint32).view(np.float32),                     # subnormal inputs
        np.exp2(np.arange(-149, 128)).astype(np.float32), -np.exp2(np.arange(-149, 128)).astype(np.float32),
        np.array([0.0, -0.0, flt_max, -flt_max, np.finfo(np.float32).tiny, 1.0, -1.0, -0.0, 0.0, -0.0], np.float32),
    ]
    v = np.concatenate(parts)
    v = v[:v.size // 8 * 8]
    r.shuffle(v)                    # every position 0..7 of a cell sees every kind of input
    assert np.isfinite(v).all() and (np.abs(v) < 2.0 ** -126).sum() > 8000 and (np.abs(v) > flt_max / 2).sum() > 4000
    assert (v == 0).sum() >= 6 and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    return v


def test_limb_cells_decode_to_the_three_limbs_of_every_element(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "cells.cpp").write_text(SRC)
    exe = str(tmp_path / "cells")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rsis_amd", "csrc"), "-o", exe, str(tmp_path / "cells.cpp")])
    v = _inputs()
    v.tofile(str(tmp_path / "in.bin"))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(str(tmp_path / "out.bin"), np.uint32).reshape(-1, 36)
    assert out.shape[0] == v.size // 8
    cells = out[:, :12].reshape(-1, 3, 4)                       # [group][limb][dword]
    ref = out[:, 12:].reshape(-1, 8, 3)                         # [group][element][limb]
    # decode: element 2m = low half of dword m, element 2m + 1 = its high half; a half is the high half of the limb's fp32 encoding
    dec = np.empty((cells.shape[0], 8, 3), np.uint32)
    for l in range(3):
        dec[:, 0::2, l] = (cells[:, l, :] & 0xFFFF) << 16
        dec[:, 1::2, l] = cells[:, l, :] & 0xFFFF0000
    np.testing.assert_array_equal(dec, ref & 0xFFFF0000)        # the cells ARE the high halves of rsis_limb_split3's limbs
    limbs = dec.view(np.float32).reshape(-1, 3)
    s = (limbs[:, 0] + limbs[:, 1]) + limbs[:, 2]               # fp32, every partial sum exact
    big = (np.abs(v) >= 2.0 ** -103) | (v == 0)
    assert big.sum() > 0.8 * v.size and (~big).sum() > 8000
    nz = big & (v != 0)
    np.testing.assert_array_equal(s[nz].view(np.uint32), v[nz].view(np.uint32))        # the sum IS the input, bit for bit
    assert (s[v == 0] == 0).all()                                                      # (+0 and -0: the value is zero)
    # the header's stated exception: below 2^-103 the dropped low bits of the last limb are worth less than 2^-126
    assert np.abs(s[~big].astype(np.float64) - v[~big].astype(np.float64)).max() < 2.0 ** -126
    # signed zeros and subnormal inputs give limbs of the value's sign or zero
    assert (limbs.astype(np.float64) * v[:, None].astype(np.float64) >= 0).all()
