"""The lane planner of the grouped bf16 / staged-limb weight-gradient launches (rsis_amd/csrc/wgrad_lanes.h: wgb_count_tiles,
wgb_plan_alone / split_plan, wgb_plan_lanes on the host, wgb_find in every block), on the CPU: the header is plain C++ and a few lines
of host code with their own main around it are compiled with the system compiler, with -fsanitize=address,undefined so that the
fixed tables of WgradBf16Group (lane_start[8][29], 16-bit splits, 8-bit jobs) are bounds-checked while they are written and read.

For each job list the program plans the launch or launches exactly as wgb_launch_bucket does (count tiles, plan, next launch from
the first job the last one did not take) and walks EVERY block index of every grid through wgb_find.  The test then asserts, from the
enumeration of (job, tile, split) itself -- not from a second run of the planner:
  * every (job, tile, split) with tile < n_co_tiles * n_n_tiles and split < ceil(n_sp_tiles / tiles_per_split) is produced exactly
    once, and every other block reports "padding";
  * the splits of a job partition [0, n_sp_tiles): tiles_per_split >= 1 and no split is empty;
  * all blocks of one (job, split) sit on one lane (blocks 8 k + x) at consecutive k, and a job is at most 8 runs of consecutive
    splits (its items), each on one lane;
  * no lane holds more than RSIS_WGB_LANE_ITEMS items, a launch holds at most RSIS_WGB_MAXJ jobs, and job and split numbers come
    back from the 8- / 16-bit tables untruncated (a truncated one would repeat or miss a triple);
  * deterministic mode: one split per job; the plain mode: exactly tiles * splits blocks, none of them padding."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXJ, LANE_ITEMS = 32, 28      # RSIS_WGB_MAXJ, RSIS_WGB_LANE_ITEMS

SRC = r"""
#include "wgrad_lanes.h"
#include <stdio.h>
#include <stdlib.h>
static FILE* o;
static void put(int v) { fwrite(&v, 4, 1, o); }
static void walk(const WgradBf16Group& g, const WgbPlan pl) {
  put(pl.blocks); put(pl.jobs); put(g.n);
  for (int x = 0; x < 8; ++x) put(g.lane_n[x]);
  for (int j = 0; j < g.n; ++j) { put(g.job[j].n_co_tiles); put(g.job[j].n_n_tiles); put(g.job[j].n_sp_tiles); put(g.job[j].tiles_per_split); }
  for (int b = 0; b < pl.blocks; ++b) {
    int job = -1, tile = -1, split = -1;
    const int found = wgb_find(g, [b] { return (unsigned)b; }, job, tile, split) ? 1 : 0;
    put(found); put(job); put(tile); put(split);
  }
}
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "r");
  o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int alone, det, bm, bn, tw, th, n;
  long target;
  while (fscanf(f, "%d %d %ld %d %d %d %d %d", &alone, &det, &target, &bm, &bn, &tw, &th, &n) == 8) {
    WgradBf16Args* jobs = (WgradBf16Args*)calloc(n, sizeof(WgradBf16Args));     // (heap: the sanitizer sees reads past the list)
    for (int j = 0; j < n; ++j)
      if (fscanf(f, "%d %d %d %d %d", &jobs[j].B, &jobs[j].Cs, &jobs[j].H, &jobs[j].W, &jobs[j].Cout) != 5) return 3;
    const long total = wgb_count_tiles(jobs, n, bm, bn, tw, th);
    WgradBf16Group* g = (WgradBf16Group*)malloc(sizeof(WgradBf16Group));
    if (alone) {
      put(1);
      const WgbPlan pl = wgb_plan_alone(*g, jobs[0], det != 0);
      walk(*g, pl);
    } else {
      int launches = 0;
      for (int j0 = 0; j0 < n; ++launches) j0 += wgb_plan_lanes(*g, jobs + j0, n - j0, total, target, det != 0).jobs;
      put(launches);
      for (int j0 = 0; j0 < n;) {
        const WgbPlan pl = wgb_plan_lanes(*g, jobs + j0, n - j0, total, target, det != 0);
        if (pl.jobs < 1) return 4;
        walk(*g, pl);
        j0 += pl.jobs;
      }
    }
    free(g);
    free(jobs);
  }
  fclose(o);
  return 0;
}
"""

# a job = (B, Cs, H, W, Cout); a key = (bm, bn, tw, th) as wgb_key gives them
K3 = (64, 32, 32, 2)         # 3x3, 32-wide tiles
K1 = (128, 128, 64, 1)       # 1x1 on the flattened map
_MIX = [(4, 64, 16, 32, 64), (2, 200, 16, 32, 136), (1, 8, 2, 32, 8), (32, 256, 56, 56, 256), (3, 40, 17, 33, 72), (8, 512, 14, 32, 512),
        (1, 32, 2, 32, 64), (16, 96, 28, 28, 48)]


def _mix(n, seed):
    r = np.random.default_rng(seed)
    return [_MIX[i % len(_MIX)] if i < len(_MIX) else
            (int(r.integers(1, 33)), int(r.integers(1, 600)), int(r.integers(1, 57)), int(r.integers(1, 57)), int(r.integers(2, 600)))
            for i in range(n)]


def _scenarios():
    s = []
    # one job alone (the plain mode), deterministic and not; tile counts of 1; few and many spatial tiles
    for det in (0, 1):
        for key, job in ((K3, (4, 64, 16, 32, 64)), (K3, (1, 8, 2, 32, 8)), (K3, (32, 256, 56, 56, 256)), (K1, (1, 64, 1, 64, 64)),
                         (K1, (32, 1024, 1, 3136, 256)), (K3, (1, 32, 4, 32, 600))):
            s.append(dict(alone=1, det=det, target=896, key=key, jobs=[job]))
    # 1, 2, 31, 32, 33 and 40 jobs at the three target block counts, deterministic and not
    for n in (1, 2, 31, 32, 33, 40):
        for target in (1, 896, 100000):
            for det in (0, 1):
                s.append(dict(alone=0, det=det, target=target, key=K3 if n % 2 else K1, jobs=_mix(n, 100 * n + det)))
    # tile counts of 1 throughout: one dW tile, one spatial tile per job
    s.append(dict(alone=0, det=0, target=896, key=K3, jobs=[(1, 8, 2, 32, 8)] * 5))
    # a job whose split count exceeds 8: 8 items of consecutive splits (1024 spatial tiles, two per block at the least)
    s.append(dict(alone=0, det=0, target=100000, key=K3, jobs=[(64, 32, 32, 32, 64)], many_splits=True))
    s.append(dict(alone=0, det=0, target=896, key=K3, jobs=[(64, 32, 32, 32, 64), (1, 8, 2, 32, 8)], many_splits=True))
    # more than 2^15 splits of one job: the 16-bit split table holds them
    s.append(dict(alone=0, det=0, target=100000, key=(64, 32, 8, 8), jobs=[(2048, 32, 64, 64, 64)], many_splits=True, min_splits=1 << 15))
    # 30 many-split jobs: 8 items each, so the 8 * RSIS_WGB_LANE_ITEMS items end the first launch at 28 jobs, not RSIS_WGB_MAXJ
    s.append(dict(alone=0, det=0, target=100000, key=K3, jobs=[(16, 32, 32, 32, 64)] * 30, item_limit=True))
    return s


def _cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("wgrad_lanes")
    (d / "lanes.cpp").write_text(SRC)
    exe = str(d / "lanes")
    base = [cxx, "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "rsis_amd", "csrc"), "-o", exe, str(d / "lanes.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    sanitized = subprocess.call(base + san) == 0
    if not sanitized:                      # (a host compiler that cannot link the sanitizers: the tables are then checked by the asserts alone)
        subprocess.check_call(base)
    print("wgrad_lanes host program built %s -fsanitize=address,undefined" % ("with" if sanitized else "WITHOUT"))
    sc = _scenarios()
    with open(str(d / "in.txt"), "w") as f:
        for s in sc:
            f.write("%d %d %d %d %d %d %d %d\n" % ((s["alone"], s["det"], s["target"]) + s["key"] + (len(s["jobs"]),)))
            for j in s["jobs"]:
                f.write("%d %d %d %d %d\n" % j)
    subprocess.check_call([exe, str(d / "in.txt"), str(d / "out.bin")])
    return sc, np.fromfile(str(d / "out.bin"), np.int32), sanitized


def _check_launch(s, jobs, blocks, lane_n, tabs, rec, plain):
    """one launch: `jobs` its job list, tabs[j] = (n_co, n_n, n_sp, tiles_per_split) as the kernel sees them, rec[b] = wgb_find of block b"""
    bm, bn, tw, th = s["key"]
    found, job, tile, split = rec[:, 0] == 1, rec[:, 1], rec[:, 2], rec[:, 3]
    assert ((rec[~found, 1:] == -1).all()), "a padding block wrote its outputs"
    if plain:
        assert lane_n[0] < 0 and found.all()
    else:
        assert (lane_n >= 0).all() and (lane_n <= LANE_ITEMS).all() and len(jobs) <= MAXJ and blocks % 8 == 0
    b = np.arange(blocks)[found]
    job, tile, split = job[found], tile[found], split[found]
    assert ((job >= 0) & (job < len(jobs))).all()
    produced = 0
    for j, (B, Cs, H, W, Cout) in enumerate(jobs):
        n_co, n_n, n_sp, tps = (int(v) for v in tabs[j])
        assert (n_co, n_n, n_sp) == (_cdiv(Cout, bm), _cdiv(Cs, bn), B * _cdiv(H, th) * _cdiv(W, tw))
        assert tps >= 1
        ntile, nsplit = n_co * n_n, _cdiv(n_sp, tps)
        assert (nsplit - 1) * tps < n_sp <= nsplit * tps                  # splits [s * tps, min((s + 1) * tps, n_sp)) partition [0, n_sp)
        if s["det"]:
            assert nsplit == 1
        if "min_splits" in s:
            assert nsplit > s["min_splits"]
        elif s.get("many_splits") and j == 0:
            assert nsplit > 8
        m = job == j
        t, sp, bj = tile[m], split[m], b[m]
        assert ((t >= 0) & (t < ntile) & (sp >= 0) & (sp < nsplit)).all(), "job %d: a tile or split out of range" % j
        assert np.array_equal(np.bincount(sp.astype(np.int64) * ntile + t, minlength=ntile * nsplit), np.ones(ntile * nsplit, np.int64)), \
            "job %d: a (tile, split) missing or repeated" % j
        produced += ntile * nsplit
        if plain:
            assert blocks == ntile * nsplit and np.array_equal(t, bj % ntile) and np.array_equal(sp, bj // ntile)
            continue
        lane, k = bj & 7, bj >> 3
        lo, hi, kmin, kmax = np.full(nsplit, 8), np.full(nsplit, -1), np.full(nsplit, 1 << 30), np.full(nsplit, -1)
        np.minimum.at(lo, sp, lane); np.maximum.at(hi, sp, lane); np.minimum.at(kmin, sp, k); np.maximum.at(kmax, sp, k)
        assert np.array_equal(lo, hi), "job %d: a split on two lanes" % j
        assert np.array_equal(kmax - kmin + 1, np.full(nsplit, ntile)), "job %d: the blocks of a split are not consecutive in their lane" % j
        runs = 1 + int(((lo[1:] != lo[:-1]) | (kmin[1:] != kmin[:-1] + ntile)).sum())     # items: runs of consecutive splits on one lane
        assert runs <= 8 and runs <= nsplit, "job %d: %d items" % (j, runs)
    assert produced == int(found.sum())


def test_every_block_of_every_grid_finds_its_triple_exactly_once(walked):
    scenarios, out, sanitized = walked
    if not sanitized:
        import warnings
        warnings.warn("the host compiler did not link -fsanitize=address,undefined: the fixed tables were not bounds-checked")
    p, seen_item_limit, seen_maxj = 0, False, False
    for s in scenarios:
        launches = int(out[p]); p += 1
        assert launches >= 1
        j0 = 0
        for _ in range(launches):
            blocks, took, gn = (int(v) for v in out[p:p + 3])
            lane_n = out[p + 3:p + 11]
            p += 11
            assert took == gn and 1 <= took <= len(s["jobs"]) - j0 and blocks >= 1
            tabs = out[p:p + 4 * gn].reshape(gn, 4); p += 4 * gn
            rec = out[p:p + 4 * blocks].reshape(blocks, 4); p += 4 * blocks
            _check_launch(s, s["jobs"][j0:j0 + took], blocks, lane_n, tabs, rec, bool(s["alone"]))
            if s.get("item_limit") and j0 == 0:
                assert took == LANE_ITEMS and (lane_n == LANE_ITEMS).all()      # 28 jobs x 8 items fill every lane: the item limit ended it
                seen_item_limit = True
            seen_maxj |= took == MAXJ and len(s["jobs"]) - j0 > MAXJ
            j0 += took
        assert j0 == len(s["jobs"]), "jobs left over"
    assert p == out.size and seen_item_limit and seen_maxj
