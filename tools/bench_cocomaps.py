"""Times the COCO label path (NOTES.md entry on rsis_paint_instance_maps, rsis_amd/csrc/cocomaps.hip):

    python tools/bench_cocomaps.py [--batch 32] [--records 7 60] [--size 256] [--T 20] [--reps 200] [--host_samples 4] [--loader_images 32]
    python tools/bench_cocomaps.py --resources          (no GPU: the compiler's resource report of the kernel)

For each record count, B samples of 480 x 640 with that many polygon records each (1 - 3 parts, 10 - 60 vertices, as
tools/bench_polymask.py draws them), painted to size x size through the tables dataloader/coco.py stages:
  paint    : the rsis_paint_instance_maps launch alone (rows and areas already on the device);
  poly     : rsis_poly_to_bits + paint -- what DeviceLoader runs per batch (device_maps);
  targets  : the same plus the grouped targets kernel (one host sync);
  stage    : the host side of the batch, COCO.stage_tables (numpy);
  host     : the alternative the other readers use, per sample on one core: numpy rasterisation of every record at native size, the
             composition of both maps and scipy's zoom(order=0) of both -- measured on `--host_samples` samples and checked equal to
             the device maps.
Device events over `--reps` launches after warm-up.  Bytes are computed from the shapes: the maps written (8 B per output pixel), the
index tables read, and the bit rows (an upper bound of what the probe can touch).
  loader   : batches/s of the DeviceLoader over a synthesized tree of 480 x 640 JPEGs, first epoch (decode) and second (decode cache),
             batch 4, -imsize 256, augmentation on.
One JSON line."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 480, 640


def resources():
    """registers / LDS / scratch of paint_maps_kernel from hipcc's -Rpass-analysis=kernel-resource-usage"""
    src = os.path.join(ROOT, "rsis_amd", "csrc", "cocomaps.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True)
    out = {}
    for key, pat in (("vgprs", r"VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"SGPRs: (\d+)"), ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"),
                     ("scratch_bytes", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
        m = re.search(pat, r.stderr)
        out[key] = int(m.group(1)) if m else None
    return out


def write_annotations(path, batch, k, seed):
    from tools.bench_polymask import make_set
    recs = make_set(batch * k, seed)
    images = [{"id": i + 1, "file_name": "%d.jpg" % i, "height": H, "width": W} for i in range(batch)]
    anns = [{"id": j + 1, "image_id": j // k + 1, "category_id": 1 + j % 80, "iscrowd": 0, "area": float(j % 977),
             "segmentation": [np.clip(p.reshape(-1, 2), 0, [W, H]).reshape(-1).tolist() for p in parts]} for j, parts in enumerate(recs)]
    os.makedirs(os.path.join(path, "annotations"), exist_ok=True)
    with open(os.path.join(path, "annotations", "instances_train2017.json"), "w") as f:
        json.dump({"images": images, "annotations": anns, "categories": [{"id": c, "name": "c%d" % c} for c in range(1, 81)]}, f)


def events_ms(fn, reps):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def one_case(a, k):
    import torch
    from scipy.ndimage import zoom
    from rsis_amd._lib import check, lib, ptr, stream
    from rsis_amd.dataloader.coco import COCO, compose_maps, polygon_mask
    from rsis_amd.dataloader.targets import targets_kernel
    from tools.bench_targets import median_ms
    d = tempfile.mkdtemp()
    write_annotations(d, a.batch, k, 11 + k)
    args = argparse.Namespace(gt_maxseqlen=a.T, batch_size=a.batch, coco_dir=d, coco_train_set="train2017", coco_val_set="val2017",
                              num_classes=81, rotation=10, translation=0.1, shear=0.1, zoom=0.7)
    ds = COCO(args, split="train", imsize=a.size, resize=True)
    S = (a.size, a.size)
    records = [(i, S, False, None) for i in range(a.batch)]
    t0 = time.perf_counter()
    for _ in range(5):
        table, lay = ds.stage_tables(records, S)
    stage_ms = (time.perf_counter() - t0) / 5 * 1e3
    td = torch.from_numpy(table).cuda()
    L, o, B, n, nw = lib(), lay["off"], lay["B"], lay["n"], lay["words"]
    xy, ptab, poly, paint, imgs = (td[o[j]:o[j + 1]] for j in range(5))
    src = td[o[5]:o[6]].view(torch.int32)
    scratch, bits = torch.empty((nw,), dtype=torch.int64, device="cuda"), torch.empty((nw,), dtype=torch.int64, device="cuda")
    area = torch.empty((n,), dtype=torch.int32, device="cuda")
    ins = torch.empty((B,) + S, dtype=torch.int32, device="cuda")
    seg = torch.empty_like(ins)

    def run_poly():
        check(L.rsis_poly_to_bits(ptr(xy), lay["nverts"], ptr(ptab), lay["nparts"], ptr(poly), n, ptr(scratch), ptr(bits), nw, ptr(area),
                                  stream()), "rsis_poly_to_bits")

    def run_paint():
        check(L.rsis_paint_instance_maps(ptr(bits), nw, ptr(area), n, ptr(paint), ptr(imgs), B, lay["max_recs"], ptr(src),
                                         ptr(src) + 4 * B * S[0], S[0], S[1], ptr(ins), ptr(seg), stream()), "rsis_paint_instance_maps")

    run_poly()
    paint_ms = events_ms(run_paint, a.reps)
    both_ms = events_ms(lambda: (run_poly(), run_paint()), max(10, a.reps // 10))
    tgt_ms = median_ms(lambda: (run_poly(), run_paint(), targets_kernel(ins, seg, a.T)), 3, 20)
    same = bool(torch.equal(ds.device_maps(td, lay)[0], ins))
    # the host alternative, per sample
    t0 = time.perf_counter()
    equal = True
    for i in range(a.host_samples):
        recs = ds.records(i)
        hi, hs = compose_maps([polygon_mask(p, H, W) for p, _i, _c in recs], [q for _p, q, _c in recs], [c for _p, _i, c in recs], H, W)
        f = [float(S[0]) / H, float(S[1]) / W]
        hi, hs = zoom(hi, f, mode="nearest", order=0), zoom(hs, f, mode="nearest", order=0)
        equal = equal and np.array_equal(hi, ins[i].cpu().numpy()) and np.array_equal(hs, seg[i].cpu().numpy())
    host_ms = (time.perf_counter() - t0) / max(1, a.host_samples) * 1e3
    out_bytes = 8 * B * S[0] * S[1]
    return {"B": B, "records_per_sample": k, "native": [H, W], "out": list(S), "paint_ms": round(paint_ms, 4),
            "poly_plus_paint_ms": round(both_ms, 4), "poly_paint_targets_ms": round(tgt_ms, 4), "stage_tables_ms": round(stage_ms, 3),
            "table_bytes": int(table.nbytes), "host_numpy_ms_per_sample": round(host_ms, 2),
            "host_numpy_ms_per_batch": round(host_ms * B, 1), "host_equals_device": bool(equal), "device_maps_equal": same,
            "bytes_written": out_bytes, "bytes_index_tables": 4 * B * (S[0] + S[1]), "bytes_bit_rows": 8 * nw,
            "paint_write_GB_per_s": round(out_bytes / paint_ms / 1e6, 1)}


def loader_rates(a):
    import torch
    from rsis_amd.dataloader.coco import COCO, synthesize_coco_dir
    from rsis_amd.dataloader.loader import DeviceLoader
    d = synthesize_coco_dir(os.path.join(tempfile.mkdtemp(), "coco"), n=a.loader_images, sizes=((H, W),), sets=("train2017",))
    args = argparse.Namespace(gt_maxseqlen=a.T, batch_size=4, coco_dir=d, coco_train_set="train2017", coco_val_set="val2017", num_classes=4,
                              rotation=10, translation=0.1, shear=0.1, zoom=0.7)
    dl = DeviceLoader(COCO(args, split="train", imsize=256, augment=True), 4, num_workers=4)
    rates = []
    for _epoch in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in dl)
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    return {"images": a.loader_images, "batch": 4, "decode_batches_per_s": round(rates[0], 3), "cached_batches_per_s": round(rates[1], 3),
            "cached_again_batches_per_s": round(rates[2], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--records", type=int, nargs="+", default=[7, 60])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host_samples", type=int, default=4)
    ap.add_argument("--loader_images", type=int, default=32)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args(argv)
    if a.resources:
        print(json.dumps({"paint_maps_kernel": resources()}))
        return
    out = {"cases": [one_case(a, k) for k in a.records]}
    if a.loader_images > 0:
        out["loader_480x640"] = loader_rates(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
