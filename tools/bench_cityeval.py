"""Times the Cityscapes pixel counting (rsis_amd/csrc/insteval.hip): 500 synthetic 1024 x 2048 images' worth of work in batches, 160
predictions each over 20 distinct masks (the result writer stores every mask under eight names; the evaluation counts each distinct mask
once, --all_masks counts all 160).  Prints the kernel time per launch and per image (presence + overlap, device events, medians), the
achieved bytes/s against the bytes the overlap launch must read (gt once per 64-mask group + the packed masks), the time per image
with the copies and the host-side lut (overlap_counts_batch end to end), and for comparison on the same host: the numpy count table
(np.unique + np.bincount) and the direct boolean-image counting of tests/cityscapes_golden.py on a few images.

    python tools/bench_cityeval.py [--images 500] [--batch 10] [--all_masks] [--host_images 2]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 1024, 2048


def scene(rng, n_inst=40, n_masks=20):
    gt = np.full((H, W), 7, np.uint16)
    for k in range(n_inst):
        h, w = int(rng.integers(20, 300)), int(rng.integers(20, 400))
        y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        gt[y:y + h, x:x + w] = int(rng.choice([24, 25, 26, 27, 28, 31, 32, 33])) * 1000 + k
    masks = np.zeros((n_masks, H, W), np.uint8)
    for k in range(n_masks):
        h, w = int(rng.integers(20, 300)), int(rng.integers(20, 400))
        y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        masks[k, y:y + h, x:x + w] = 255
    return gt, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--all_masks", action="store_true", help="count all 160 prediction lines' masks instead of the 20 distinct ones")
    ap.add_argument("--host_images", type=int, default=2)
    a = ap.parse_args()
    from rsis_amd import cityscapes_eval as E
    from rsis_amd._lib import check, lib, ptr, stream
    import cityscapes_cases as C
    import cityscapes_golden as G
    L = lib()
    rng = np.random.default_rng(0)
    distinct = [scene(rng) for _ in range(min(a.batch, 4))]
    if a.all_masks:
        distinct = [(g, np.repeat(m, 8, 0)) for g, m in distinct]
    gts = [distinct[i % len(distinct)][0] for i in range(a.batch)]
    sets = [distinct[i % len(distinct)][1] for i in range(a.batch)]
    P = len(sets[0])
    want = C.np_counts(gts[0], sets[0])
    got = E.overlap_counts_batch(gts, sets)
    assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[0][1], want[1])
    launches = -(-a.images // a.batch)
    # end to end: pool copy, presence, lut, overlap, copy back
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        E.overlap_counts_batch(gts, sets)
    torch.cuda.synchronize()
    e2e = (time.perf_counter() - t0) / (launches * a.batch)
    # the two launches alone, resident inputs
    dev = torch.device("cuda")
    S = [len(g[1]) for g in got]
    jobs, length, blk, pblk, cnt = E.job_table([H * W] * a.batch, [P] * a.batch, S)
    pool = torch.zeros((length,), dtype=torch.uint8)
    lut = np.full((a.batch, 65536), 65535, np.uint16)
    for j, g in enumerate(gts):
        pool[jobs[j, 0]:jobs[j, 0] + 2 * H * W] = torch.from_numpy(g.reshape(-1).view(np.uint8))
        lut[j, got[j][1]] = np.arange(S[j])
    pool, dlut, dj = pool.to(dev), torch.from_numpy(lut.view(np.int16)).to(dev), torch.from_numpy(jobs).to(dev)
    bits = torch.cat([E._pack_masks(m, (H, W), "m", dev)[0] for m in sets])
    counts = torch.empty((cnt,), dtype=torch.int32, device=dev)
    flags = torch.empty((a.batch * 65536,), dtype=torch.uint8, device=dev)

    def presence():
        check(L.rsis_inst_presence_batch(ptr(pool), pool.numel(), ptr(dj), a.batch, pblk, ptr(flags), flags.numel(), stream()), "presence")

    def overlap():
        check(L.rsis_inst_overlap_batch(ptr(pool), pool.numel(), ptr(dj), a.batch, blk, ptr(dlut), dlut.numel(), ptr(bits), bits.numel(),
                                        ptr(counts), counts.numel(), stream()), "overlap")

    def timed(fn, reps):
        for _ in range(5):
            fn()
        ms = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms.append(s.elapsed_time(e))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))
    reps = max(20, launches)
    pm, ov = timed(presence, reps), timed(overlap, reps)
    groups = max(1, -(-P // 64))
    must = a.batch * (2 * H * W * groups + P * (H * W // 8))
    print("batch %d images of %d x %d, %d masks each (%d groups), %d launches timed" % (a.batch, H, W, P, groups, reps))
    print("presence launch : median %.3f ms (min %.3f, max %.3f) = %.4f ms / image" % (pm + (pm[0] / a.batch,)))
    print("overlap launch  : median %.3f ms (min %.3f, max %.3f) = %.4f ms / image, %.1f GB/s of the %.1f MB it must read"
          % (ov + (ov[0] / a.batch, must / ov[0] / 1e6, must / 1e6)))
    print("with copies + lut (overlap_counts_batch, host arrays in, host tables out): %.3f ms / image; %d images: %.2f s"
          % (e2e * 1e3, a.images, e2e * a.images))
    t0 = time.perf_counter()
    for i in range(a.host_images):
        C.np_counts(gts[i % a.batch], sets[i % a.batch])
    t_np = (time.perf_counter() - t0) / max(1, a.host_images)
    t0 = time.perf_counter()
    for i in range(a.host_images):
        G.direct_counts(gts[i % a.batch], sets[i % a.batch])
    t_dir = (time.perf_counter() - t0) / max(1, a.host_images)
    print("host, same inputs: numpy count table (np.unique + np.bincount) %.1f ms / image; direct boolean images (golden module) %.1f ms / image"
          % (t_np * 1e3, t_dir * 1e3))


if __name__ == "__main__":
    main()
