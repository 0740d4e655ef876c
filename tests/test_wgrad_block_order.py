"""The block order of the grouped fp32 weight-gradient launch (rsis_amd/csrc/wgrad_block_order.h), on the CPU: the header is plain C++,
a few lines of host code around rsis_xcd_logical_block are compiled with the system compiler.  For a launch of N blocks the map from
the hardware block index to the logical one must be a bijection on [0, N), and the blocks b, b + 8, ... (the ones that share an XCD)
must receive increasing, contiguous logical indices: XCD x owns one range, and the eight ranges tile [0, N) in the order of x."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "wgrad_block_order.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const int n = atoi(argv[i]);
    printf("%d", n);
    for (int b = 0; b < n; ++b) printf(" %d", rsis_xcd_logical_block(b, n));
    printf("\n");
  }
  return 0;
}
"""

SIZES = list(range(1, 71)) + [2047, 2048, 2049, 4099] + [1000 + r for r in range(8)]


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("block_order")
    (d / "order.cpp").write_text(SRC)
    exe = str(d / "order")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rsis_amd", "csrc"), "-o", exe, str(d / "order.cpp")])
    out = subprocess.check_output([exe] + [str(n) for n in SIZES]).decode().splitlines()
    res = {}
    for line in out:
        v = [int(t) for t in line.split()]
        res[v[0]] = np.array(v[1:], np.int64)
    assert sorted(res) == sorted(set(SIZES))
    return res


def test_every_remainder_is_covered():
    assert {n % 8 for n in SIZES if n >= 8} == set(range(8)) and {n % 8 for n in SIZES if n > 1000} == set(range(8))


@pytest.mark.parametrize("n", SIZES)
def test_map_is_a_bijection(maps, n):
    m = maps[n]
    assert m.size == n
    np.testing.assert_array_equal(np.sort(m), np.arange(n))
    if n < 8:
        np.testing.assert_array_equal(m, np.arange(n))       # fewer blocks than XCDs: one block each, the identity


@pytest.mark.parametrize("n", SIZES)
def test_blocks_of_one_xcd_get_one_contiguous_increasing_range(maps, n):
    m = maps[n]
    start = 0
    for x in range(min(8, n)):
        mine = m[x::8]                                         # blocks x, x + 8, ...: in the order the XCD runs them
        assert mine.size == n // 8 + (1 if x < n % 8 else 0)
        np.testing.assert_array_equal(mine, start + np.arange(mine.size))
        start += mine.size
    assert start == n
