"""Times the Cityscapes label path (NOTES.md entry on rsis_instance_maps):

    python tools/bench_instmaps.py [--batch 32] [--height 256] [--width 512] [--T 20] [--instances 20] [--runs 20] [--loader_images 8]

  maps     : rsis_instance_maps alone (raw ids -> class map + compact instance map);
  kernel   : maps + the grouped targets kernel (one host sync per batch) -- the path of dataloader/cityscapes.py;
  loop     : the only path the raw ids had before: dataloader.targets_from_maps on the raw ids, which the grouped kernel refuses
             (ids above 255), i.e. the per-image loop with one torch.unique host sync per image (the class map is handed to it
             ready-made, which flatters it);
  loader   : batches/s of the DeviceLoader over a synthesized tree of `--loader_images` 1024 x 2048 images, first epoch (PNG decode)
             and second epoch (decode cache), batch 4, -imsize 256.
HIP events around each call (they span the host syncs inside it), `--warmup` calls first, the median of `--runs`.  One JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_targets import median_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--instances", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--loader_images", type=int, default=8)
    a = ap.parse_args(argv)
    from rsis_amd.dataloader.cityscapes import CityScapes, maps_from_ids, synthesize_cityscapes_dir
    from rsis_amd.dataloader.loader import DeviceLoader
    from rsis_amd.dataloader.targets import targets_from_maps
    r = np.random.default_rng(0)
    B, H, W = a.batch, a.height, a.width
    labels = np.array([24, 25, 26, 27, 28, 31, 32, 33])
    pool = np.concatenate([[7], labels[r.integers(0, 8, a.instances)] * 1000 + np.arange(a.instances)])
    coarse = pool[r.integers(0, len(pool), (B, 16, 16))]                   # blocks of a coarse grid: areas differ
    raw = torch.from_numpy(np.kron(coarse, np.ones((H // 16, W // 16), np.int64)).astype(np.int32)).cuda()
    maps = median_ms(lambda: maps_from_ids(raw), a.warmup, a.runs)
    kern = median_ms(lambda: targets_from_maps(*maps_from_ids(raw), a.T), a.warmup, a.runs)
    ins, seg = maps_from_ids(raw)
    loop = median_ms(lambda: targets_from_maps(raw, seg, a.T), a.warmup, max(3, a.runs // 4))
    same = all(torch.equal(p, q) for p, q in zip(targets_from_maps(raw, seg, a.T), targets_from_maps(ins, seg, a.T)))
    out = {"targets": {"B": B, "H": H, "W": W, "T": a.T, "instances": a.instances, "maps_ms": round(maps, 4),
                       "maps_plus_targets_ms": round(kern, 4), "loop_ms": round(loop, 4), "speedup": round(loop / kern, 2),
                       "bit_equal": bool(same)}}
    if a.loader_images > 0:
        d = synthesize_cityscapes_dir(os.path.join(tempfile.mkdtemp(), "cs"), n=a.loader_images, sizes=((1024, 2048),))
        args = argparse.Namespace(gt_maxseqlen=a.T, batch_size=4, cityscapes_dir=d, rotation=10, translation=0.1, shear=0.1, zoom=0.7,
                                  crop=False)
        dl = DeviceLoader(CityScapes(args, split="train", imsize=256, augment=True), 4, num_workers=4)
        rates = []
        for _epoch in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(1 for _ in dl)
            torch.cuda.synchronize()
            rates.append(n / (time.perf_counter() - t0))
        out["loader_1024x2048"] = {"images": a.loader_images, "batch": 4, "decode_batches_per_s": round(rates[0], 3),
                                   "cached_batches_per_s": round(rates[1], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
