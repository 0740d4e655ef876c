"""Shared by the Cityscapes evaluation tests: the fixture's cases, a numpy count table and a results-folder writer."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "cityscapes.npz")
ROAD = 7


def load_cases():
    """-> list of cases; a case = {"images": [dict of the per-image arrays], "aps", "all", "cls"}"""
    z = np.load(FIXTURE)
    cases = []
    for k in range(int(z["ncases"])):
        images = []
        for i in range(int(z["c%d_n" % k])):
            pre = "c%d_i%d_" % (k, i)
            images.append({key[len(pre):]: z[key] for key in z.files if key.startswith(pre)})
        cases.append({"images": images, "aps": z["c%d_aps" % k], "all": z["c%d_all" % k], "cls": z["c%d_cls" % k]})
    return cases


def np_counts(gt, masks):
    """(P + 1, S) int64 count table and the sorted ids with np.unique + np.bincount"""
    ids, inv = np.unique(np.asarray(gt).reshape(-1), return_inverse=True)
    inv = inv.reshape(-1)
    rows = [np.bincount(inv[np.asarray(m).reshape(-1) != 0], minlength=len(ids)) for m in masks]
    rows.append(np.bincount(inv, minlength=len(ids)))
    return np.stack(rows).astype(np.int64), ids.astype(np.int64)


def np_counts_batch(gt_images, mask_sets):
    return [np_counts(g, m) for g, m in zip(gt_images, mask_sets)]


def full_counts(img):
    """the fixture's table of DISTINCT masks -> one row per line + the histogram"""
    return np.concatenate([img["counts"][img["rows"]], img["counts"][-1:]])


def write_folder(root, images, distinct_names=False):
    """the images of a case as a results folder + a ground-truth tree: <root>/results/<stem>.txt, masks under results/masks/ (one file
    per LINE, so the same mask is stored under several names, as the result writer does), gt under <root>/gt/city<i>/."""
    from PIL import Image
    res, gt_dir = os.path.join(root, "results"), os.path.join(root, "gt")
    os.makedirs(os.path.join(res, "masks"), exist_ok=True)
    for i, img in enumerate(images):
        stem = "city%d_%06d_000019" % (i, i)
        os.makedirs(os.path.join(gt_dir, "city%d" % i), exist_ok=True)
        Image.fromarray(img["gt"].astype(np.uint16)).save(os.path.join(gt_dir, "city%d" % i, stem + "_gtFine_instanceIds.png"))
        lines = []
        for q, (r, lab, sc) in enumerate(zip(img["rows"], img["labels"], img["scores"])):
            name = "masks/%s_%d.png" % (stem, q)
            Image.fromarray((img["masks"][r] * np.uint8(255)).astype(np.uint8), mode="L").save(os.path.join(res, name))
            lines.append("%s %d %r\n" % (name, lab, float(sc)))
        with open(os.path.join(res, stem + ("_leftImg8bit" if i % 2 else "") + ".txt"), "w") as f:
            f.writelines(lines)
    return res, gt_dir
