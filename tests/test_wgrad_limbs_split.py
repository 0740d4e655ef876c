"""The three-limb split of the fp32 weight gradients' limb loop (rsis_amd/csrc/limb_split.h), on the CPU: the header is plain C++, a few
lines of host code around rsis_limb_split3 are compiled with the system compiler.  For every input the limbs must add up to the
input bit for bit (l0 + l1, then + l2, in fp32: every partial sum is exact) and each limb must be a bf16 value (low 16 bits zero).
The expected answer is the input itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "limb_split.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  float v;
  while (fread(&v, 4, 1, f) == 1) {
    float l[4];
    rsis_limb_split3(v, l[0], l[1], l[2]);
    volatile float s01 = l[0] + l[1];
    volatile float s = s01 + l[2];
    l[3] = s;
    fwrite(l, 4, 4, o);
  }
  fclose(o);
  return 0;
}
"""


def _inputs():
    r = np.random.default_rng(20260)
    flt_max = np.finfo(np.float32).max
    parts = [
        r.normal(0, 1, 400000).astype(np.float32),
        (r.normal(0, 1, 200000) * np.exp2(r.integers(-100, 100, 200000))).astype(np.float32),
        r.integers(0, 0x7F800000, 200000, dtype=np.int64).astype(np.uint32).view(np.float32),                    # any finite positive encoding
        (r.integers(0, 0x7F800000, 100000, dtype=np.int64) | 0x80000000).astype(np.uint32).view(np.float32),     # ... negative
        (flt_max * r.uniform(0.5, 1.0, 40000) * r.choice([-1.0, 1.0], 40000)).astype(np.float32),                # within a factor 2 of FLT_MAX
        (r.uniform(0.1, 1.0, 40000) * np.exp2(r.integers(-149, -100, 40000)) * r.choice([-1.0, 1.0], 40000)).astype(np.float32),   # below 1e-30, subnormals included
        (r.uniform(1.0, 8.0, 20000) * 2.0 ** -103 * r.choice([-1.0, 1.0], 20000)).astype(np.float32),            # below 1e-30, all residuals normal
        np.exp2(np.arange(-149, 128)).astype(np.float32), -np.exp2(np.arange(-149, 128)).astype(np.float32),     # powers of two
        np.array([0.0, -0.0, flt_max, -flt_max, np.finfo(np.float32).tiny, 1.0, -1.0], np.float32),
    ]
    v = np.concatenate(parts)
    assert v.size >= 1000000 - 20000 and np.isfinite(v).all()
    assert (np.abs(v) < 1e-30).sum() > 30000 and (np.abs(v) > flt_max / 2).sum() > 30000 and (v < 0).sum() > 100000
    return v


def test_three_limbs_add_up_to_the_value_bit_for_bit(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "split.cpp").write_text(SRC)
    exe = str(tmp_path / "split")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rsis_amd", "csrc"), "-o", exe, str(tmp_path / "split.cpp")])
    v = _inputs()
    v.tofile(str(tmp_path / "in.bin"))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(str(tmp_path / "out.bin"), np.float32).reshape(-1, 4)
    assert out.shape[0] == v.size
    bits = out.view(np.uint32)
    # each limb is a bf16 value -- wherever every residual is a NORMAL fp32 number, |v| >= 2^-103 (below, the last residual is a
    # subnormal whose low bits the pack drops: less than 2^-126 in absolute terms, see limb_split.h)
    big = (np.abs(v) >= 2.0 ** -103) | (v == 0)
    assert big.sum() > 900000 and ((np.abs(v) < 1e-30) & big & (v != 0)).sum() > 1000
    assert (bits[big][:, :3] & 0xFFFF).max() == 0, "a limb is not a bf16 value"
    dropped = (bits[~big][:, :3] & 0xFFFF).view(np.float32)
    assert np.abs(dropped).max() < 2.0 ** -126
    np.testing.assert_array_equal(bits[:, 3][v != 0], v.view(np.uint32)[v != 0])       # the sum IS the input, bit for bit
    assert (out[:, 3][v == 0] == 0).all()                                              # (+0 and -0: 0 - 0 = +0, the value is zero)
    # limbs carry the sign of the value or are zero, and each is below 2^-7 of the one before
    assert (out[:, :3] * v[:, None] >= 0).all()
    a, av = np.abs(out[:, :3].astype(np.float64)), np.abs(v.astype(np.float64))
    assert (a[:, 0] <= av).all() and (a[:, 1] * 2.0 ** 7 <= av).all() and (a[big, 2] * 2.0 ** 14 <= av[big]).all()
