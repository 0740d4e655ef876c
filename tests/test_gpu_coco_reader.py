"""COCO on the device: rsis_paint_instance_maps against its numpy statement (tests/coco_reader_cases.py), the DeviceLoader on a
synthesized tree against the host pipeline of the other readers, `train.py -dataset coco` and `eval.py -dataset coco`.  Every comparison
is exact: the kernel works on integers."""
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_reader_cases as C  # noqa: E402
import polymask_golden as PG  # noqa: E402
from test_coco_reader_host import _args  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_INS, POISON_SEG = -77, 12345


def _tables(samples, areas=None):
    """samples: [(masks, sizes, instance ids, class ids)] -> host tables (bits, area, recs, imgs) of the painter"""
    bits, area, recs, imgs, fw, k = [], [], [], [], 0, 0
    for masks, sizes, iids, cls in samples:
        imgs.append((k, len(masks)))
        for m, (h, w), i, c in zip(masks, sizes, iids, cls):
            row = C.pack(np.asarray(m, np.uint8))
            bits.append(row)
            area.append(int(np.asarray(m).sum()))
            recs.append((fw, len(row), h, w, i, c, 0, 0))
            fw += len(row)
            k += 1
    if areas is not None:
        area = list(areas)
    return (np.concatenate(bits) if bits else np.zeros((0,), np.int64), np.asarray(area, np.int32),
            np.asarray(recs, np.int64).reshape(-1, 8), np.asarray(imgs, np.int64).reshape(-1, 2))


def _launch(bits, area, recs, imgs, src_y, src_x, max_recs=None, outs=None):
    """one call on device copies of the tables -> (rc, ins, seg) with ins / seg poisoned before the call"""
    from rsis_amd._lib import lib, ptr, stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    B, Ho, Wo = len(imgs), src_y.shape[1], src_x.shape[1]
    bd, ad, rd, idv, yd, xd = dev(bits), dev(area), dev(recs), dev(imgs), dev(src_y.astype(np.int32)), dev(src_x.astype(np.int32))
    if outs is None:
        outs = (torch.full((B, Ho, Wo), POISON_INS, dtype=torch.int32, device="cuda"),
                torch.full((B, Ho, Wo), POISON_SEG, dtype=torch.int32, device="cuda"))
    if max_recs is None:
        max_recs = int(imgs[:, 1].max()) if len(imgs) else 0
    rc = lib().rsis_paint_instance_maps(ptr(bd) if bd.numel() else None, bd.numel(), ptr(ad) if ad.numel() else None, len(recs),
                                        ptr(rd) if rd.numel() else None, ptr(idv), B, max_recs, ptr(yd), ptr(xd), Ho, Wo, ptr(outs[0]),
                                        ptr(outs[1]), stream())
    torch.cuda.synchronize()
    return rc, outs[0].cpu().numpy(), outs[1].cpu().numpy()


def _check(samples, src_y, src_x, **kw):
    """the call on `samples` equals paint_rule sample by sample; returns the maps"""
    rc, ins, seg = _launch(*_tables(samples), src_y, src_x, **kw)
    assert rc == 0
    for b, (masks, sizes, iids, cls) in enumerate(samples):
        want = C.paint_rule(masks, sizes, iids, cls, src_y[b], src_x[b])
        assert np.array_equal(ins[b], want[0]) and np.array_equal(seg[b], want[1]), b
    return ins, seg


def _identity(hw):
    return np.arange(hw[0], dtype=np.int32)[None], np.arange(hw[1], dtype=np.int32)[None]


@pytest.fixture(scope="module")
def eval_set():
    """the `eval` set of polymask.npz: samples with host masks, and the SAME rows as rsis_poly_to_bits / rsis_rle_to_bits leave them"""
    from rsis_amd import cocoeval as CE
    E = PG.load()["eval"]
    samples = C.eval_samples()
    rows, areas = [], []
    for im in E["images"]:
        for r in (r for r in E["gt_poly"] if r["image_id"] == im["id"]):
            seg, n = r["segmentation"], im["height"] * im["width"]
            if isinstance(seg, dict):
                row, a = CE.rle_to_bits([np.asarray(seg["counts"], np.uint32)], [n])
            else:
                row, a = CE.poly_to_bits([seg], [(im["height"], im["width"])])
            rows.append(row[0].cpu().numpy())
            areas.append(int(a.cpu()[0]))
    return samples, rows, areas


def test_eval_set_is_what_the_issue_says_and_the_packed_rows_are_the_device_rows(eval_set):
    samples, rows, areas = eval_set
    assert len(samples) == 6 and {s[4] for s in samples} >= {(33, 47), (64, 64)}
    bits, area, recs, _imgs = _tables([s[:4] for s in samples])
    assert np.array_equal(np.concatenate(rows), bits) and areas == area.tolist()
    pairs = []
    for masks, _sizes, _iids, _cls, (h, w) in samples:
        m2 = [m.reshape(w, h).T > 0 for m in masks]
        pairs.append(sum(1 for a in range(len(m2)) for b in range(a + 1, len(m2)) if (m2[a] & m2[b]).any()))
    assert sum(pairs) >= 15 and sum(1 for p in pairs if p >= 3) >= 4 and sum(len(s[0]) for s in samples) == len(recs)


@pytest.mark.parametrize("mode", ["native", "16x16", "17x13", "96x80", "flip", "crop"])
def test_painter_on_the_eval_set(eval_set, mode):
    samples = eval_set[0]
    if mode == "native":                                       # identity tables: one call per image (the sizes differ)
        for s in samples:
            sy, sx = _identity(s[4])
            ins, _seg = _check([s[:4]], sy, sx)
            assert len(np.unique(ins)) == len(s[0]) + 1                        # every record of the set stays visible somewhere
        return
    size = {"16x16": (16, 16), "17x13": (17, 13), "96x80": (96, 80), "flip": (40, 36), "crop": (40, 40)}[mode]
    tabs = [C.ramp_tables(s[4], size) for s in samples]
    sy, sx = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
    if mode == "flip":
        sx = sx[:, ::-1]
    if mode == "crop":
        sy, sx = sy[:, 5:29], sx[:, 9:33]
    if mode == "96x80":
        assert all(len(set(t[0].tolist())) < 96 for t in tabs)               # repeated indices
    ins, seg = _check([s[:4] for s in samples], sy, sx)
    assert ins.shape == (6,) + (sy.shape[1], sx.shape[1]) and (ins > 0).any() and ((ins == 0) == (seg == 0)).all()


def _rect(hw, y0, y1, x0, x1):
    m = np.zeros(hw, np.uint8)
    m[y0:y1, x0:x1] = 1
    return m.T.reshape(-1)


def test_tie_nested_and_zero_area():
    from rsis_amd import cocoeval as CE
    hw = (20, 24)
    sy, sx = _identity(hw)
    a, b = _rect(hw, 2, 10, 2, 10), _rect(hw, 6, 14, 6, 14)                    # equal areas, overlapping
    ins, _ = _check([([a, b], [hw] * 2, [1, 2], [5, 6])], sy, sx)
    assert (ins[0, 6:10, 6:10] == 1).all() and (ins[0, 10:14, 10:14] == 2).all()
    ins, _ = _check([([b, a], [hw] * 2, [1, 2], [5, 6])], sy, sx)
    assert (ins[0, 6:10, 6:10] == 1).all() and (ins[0, 2:6, 2:6] == 2).all()
    big, small = _rect(hw, 1, 19, 1, 23), _rect(hw, 8, 11, 9, 13)              # a small object on a large one, in either order
    for order in ((0, 1), (1, 0)):
        ms = [[big, small][k] for k in order]
        ins, seg = _check([(ms, [hw] * 2, [1, 2], [3, 4])], sy, sx)
        assert (ins[0, 8:11, 9:13] == 1 + order.index(1)).all() and (ins[0, 1, 1] == 1 + order.index(0))
    # a polygon outside the image: the row rsis_poly_to_bits leaves has area 0; it never wins
    rows, area = CE.poly_to_bits([[[30.0, 2.0, 40.0, 2.0, 40.0, 10.0]], [[1.0, 1.0, 9.0, 1.0, 9.0, 9.0, 1.0, 9.0]]], [hw, hw])
    assert area.cpu().tolist()[0] == 0 and area.cpu().tolist()[1] > 0
    inside = PG.record_mask([np.array([1.0, 1.0, 9.0, 1.0, 9.0, 9.0, 1.0, 9.0])], *hw)
    assert np.array_equal(rows[1].cpu().numpy(), C.pack(inside)) and not rows[0].cpu().numpy().any()
    _check([([np.zeros(20 * 24, np.uint8), inside], [hw] * 2, [1, 2], [7, 8])], sy, sx)
    # ... and a row with bits set whose stated area is 0 does not win either
    bits, _area, recs, imgs = _tables([([a, big], [hw] * 2, [1, 2], [5, 6])])
    rc, ins, seg = _launch(bits, np.asarray([0, int(big.sum())], np.int32), recs, imgs, sy, sx)
    want = C.paint_rule([big], [hw], [2], [6], sy[0], sx[0])
    assert rc == 0 and np.array_equal(ins[0], want[0]) and np.array_equal(seg[0], want[1])


@pytest.mark.parametrize("hw", [(1, 37), (41, 1), (257, 3), (1, 1)], ids=["h1", "w1", "h257", "1x1"])
def test_thin_images_and_a_column_that_straddles_words(hw):
    r = np.random.default_rng(hw[0] * 7 + hw[1])
    masks = [(r.random(hw[0] * hw[1]) < p).astype(np.uint8) for p in (0.7, 0.4, 0.2)]
    masks[0][-1] = masks[1][-1] = 1                                            # the last element of the image
    sy, sx = _identity(hw)
    ins, _ = _check([(masks, [hw] * 3, [1, 2, 3], [9, 8, 7])], sy, sx)
    assert ins[0, -1, -1] > 0
    size = (5, 9)                                                              # and resampled up: repeated indices
    ty, tx = C.ramp_tables(hw, size)
    _check([(masks, [hw] * 3, [1, 2, 3], [9, 8, 7])], ty[None], tx[None])


def test_a_sample_without_records_and_255_records():
    sy, sx = np.arange(35, dtype=np.int32)[None], np.arange(50, dtype=np.int32)[None]
    rc, ins, seg = _launch(*_tables([([], [], [], [])]), sy, sx)              # nrec == 0: null tables
    assert rc == 0 and not ins.any() and not seg.any() and ins.shape == (1, 35, 50)
    hw = (32, 40)
    r = np.random.default_rng(5)
    masks = []
    for _k in range(255):
        y, x, a, b = int(r.integers(0, 28)), int(r.integers(0, 36)), int(r.integers(1, 5)), int(r.integers(1, 5))
        masks.append(_rect(hw, y, y + a, x, x + b))
    iy, ix = _identity(hw)
    ins, seg = _check([(masks, [hw] * 255, list(range(1, 256)), [1000 + k for k in range(255)])], iy, ix)
    assert ins.max() >= 200 and ((seg - 999 == ins) | (ins == 0)).all()
    # an empty sample between two others
    small = (masks[:3], [hw] * 3, [1, 2, 3], [4, 5, 6])
    ins, _ = _check([small, ([], [], [], []), small], np.repeat(iy, 3, 0), np.repeat(ix, 3, 0))
    assert not ins[1].any() and np.array_equal(ins[0], ins[2])


def test_mixed_native_sizes_in_one_call_equal_single_calls(eval_set):
    samples = [s[:4] for s in eval_set[0][:3]]
    sizes = [s[4] for s in eval_set[0][:3]]
    assert len(set(sizes)) >= 2
    tabs = [C.ramp_tables(hw, (30, 44)) for hw in sizes]
    sy, sx = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
    ins, seg = _check(samples, sy, sx)
    for b in range(3):
        one_i, one_s = _check([samples[b]], sy[b:b + 1], sx[b:b + 1])
        assert np.array_equal(one_i[0], ins[b]) and np.array_equal(one_s[0], seg[b])


def test_entries_out_of_range(eval_set):
    s = eval_set[0][0]
    h, w = s[4]
    sy = np.array([[-1, 0, h - 1, h, 2 ** 31 - 1, -2 ** 31, 3, 4]], np.int64).astype(np.int32)
    sx = np.array([[0, w, -5, w - 1, 2, 2 ** 30, 1]], np.int64).astype(np.int32)
    ins, seg = _check([s[:4]], sy, sx)
    assert not ins[0, [0, 3, 4, 5]].any() and not ins[0][:, [1, 2, 5]].any()
    # records that do not fit the stated lengths, or carry an id outside 1..255, are skipped; so is an image entry that does not fit
    bits, area, recs, imgs = _tables([s[:4], s[:4]])
    n = len(s[0])
    iy, ix = _identity((h, w))
    iy, ix = np.repeat(iy, 2, 0), np.repeat(ix, 2, 0)
    bad = recs.copy()
    bad[0, 0] = len(bits) - 1                                                  # first word + words runs past bits_len
    bad[1, 1] = 1                                                              # fewer words than h * w bits
    bad[2, 4] = 256
    bad[n, 4] = 0
    rc, ins, seg = _launch(bits, area, bad, imgs, iy, ix)
    want0 = C.paint_rule(s[0][3:], s[1][3:], s[2][3:], s[3][3:], iy[0], ix[0])
    want1 = C.paint_rule(s[0][1:], s[1][1:], s[2][1:], s[3][1:], iy[1], ix[1])
    assert rc == 0 and np.array_equal(ins[0], want0[0]) and np.array_equal(seg[0], want0[1])
    assert np.array_equal(ins[1], want1[0]) and np.array_equal(seg[1], want1[1])
    for entry in ((n, n + 1), (-1, 2), (0, -1), (2 * n, 1)):
        im2 = imgs.copy()
        im2[1] = entry
        rc, ins, seg = _launch(bits, area, recs, im2, iy, ix, max_recs=n)
        assert rc == 0 and not ins[1].any() and not seg[1].any() and ins[0].any()
    rc, ins, seg = _launch(bits, area, recs, imgs, iy, ix, max_recs=n - 1)     # more records than the caller's bound: 0 records
    assert rc == 0 and not ins.any() and not seg.any()


def test_refusals_write_nothing():
    from rsis_amd._lib import lib, ptr, stream
    L = lib()
    hw = (8, 8)
    bits, area, recs, imgs = _tables([([_rect(hw, 0, 4, 0, 4)] * 2, [hw] * 2, [1, 2], [1, 1])])
    sy, sx = _identity(hw)
    rc, ins, seg = _launch(bits, area, recs, imgs, sy, sx, max_recs=256)
    assert rc == 3 and (ins == POISON_INS).all() and (seg == POISON_SEG).all()
    rc, ins, seg = _launch(bits, area, recs, imgs, sy, sx, max_recs=255)
    assert rc == 0 and (ins[0, :4, :4] == 1).all()
    t = lambda a: torch.from_numpy(a).cuda()                                   # noqa: E731
    bd, ad, rd, idv, yd, xd = t(bits), t(area), t(recs), t(imgs), t(sy), t(sx)
    oi = torch.full((1, 8, 8), POISON_INS, dtype=torch.int32, device="cuda")
    os_ = torch.full((1, 8, 8), POISON_SEG, dtype=torch.int32, device="cuda")
    good = [ptr(bd), bd.numel(), ptr(ad), 2, ptr(rd), ptr(idv), 1, 2, ptr(yd), ptr(xd), 8, 8, ptr(oi), ptr(os_), stream()]
    for k in (0, 2, 4, 5, 8, 9, 12, 13):                                       # every pointer, null in turn
        a = list(good)
        a[k] = None
        assert L.rsis_paint_instance_maps(*a) == 1, k
    for k, v, want in ((13, ptr(oi), 1), (12, ptr(yd), 1), (13, ptr(bd), 1), (6, 0, 1), (10, 0, 1), (11, -1, 1), (7, -1, 1), (3, -1, 1),
                       (6, 65536, 3), (7, 256, 3)):
        a = list(good)
        a[k] = v
        assert L.rsis_paint_instance_maps(*a) == want, (k, v)
    a = list(good)
    a[10], a[11] = 65536, 32768                                                # Ho * Wo == 2^31
    assert L.rsis_paint_instance_maps(*a) == 3
    torch.cuda.synchronize()
    assert (oi == POISON_INS).all() and (os_ == POISON_SEG).all()
    assert L.rsis_paint_instance_maps(*good) == 0


@pytest.fixture(scope="module")
def coco_tree(tmp_path_factory):
    from rsis_amd.dataloader.coco import synthesize_coco_dir
    return synthesize_coco_dir(str(tmp_path_factory.mktemp("coco") / "COCO"), n=4, sizes=((48, 64), (75, 50), (33, 47)), seed=6)


def _annotation(tree, name):
    with open(os.path.join(tree, "annotations", "instances_%s.json" % name)) as f:
        return json.load(f)


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
def test_device_loader_batch_equals_the_host_pipeline(coco_tree, augment):
    """-imsize 32, batch 3: x is the normalised (warped) crop of the PIL resize; the targets are exactly sequence_from_masks of the maps
    the host pipeline of the other readers makes (compose at native size -> zoom of both -> flip -> crop -> the same warp)"""
    from PIL import Image
    from rsis_amd.dataloader import sequence_from_masks
    from rsis_amd.dataloader.augment import affine_nearest
    from rsis_amd.dataloader.coco import COCO
    from rsis_amd.dataloader.loader import MEAN, STD, DeviceLoader
    S, T, seed = 32, 20, 5
    ann = _annotation(coco_tree, "train2017")
    ds = COCO(_args(coco_tree), split="train", imsize=S, augment=augment)
    dl = DeviceLoader(ds, 3, shuffle=False, num_workers=2, seed=seed)
    assert len(dl) == 1 and ds.crop is True
    random.seed(11)                                           # RandomAffine draws from python's global stream, as the reference does
    x, y_mask, y_class, sw_mask, sw_class = next(iter(dl))
    torch.cuda.synchronize()
    rng = random.Random(seed * 1000003 + 1)                   # the loader's per-sample stream of rank 0
    seeds = [rng.getrandbits(32) for _ in range(3)]
    mats = None
    if augment:
        random.seed(11)
        mats = torch.stack([ds.augmentation_transform.matrix(S, S) for _ in range(3)])
    ims, inss, segs, moved = [], [], [], False
    for i, sd in enumerate(seeds):
        r = random.Random(sd)
        h, w = ds.raw_size(i)
        rh, rw = (S, max(S, int(S * w / h))) if w > h else (max(S, int(S * h / w)), S)
        flip = bool(augment and r.random() < 0.5)
        ow = 0 if (rw - S) // 2 <= 0 else r.randrange((rw - S) // 2)
        oh = 0 if (rh - S) // 2 <= 0 else r.randrange((rh - S) // 2)
        moved |= flip or ow > 0 or oh > 0
        with Image.open(ds.image_path(i)) as im:
            a = np.asarray(im.convert("RGB").resize((rw, rh), Image.BILINEAR)).transpose(2, 0, 1)
        a = a[:, :, ::-1] if flip else a
        ims.append(np.ascontiguousarray(a[:, oh:oh + S, ow:ow + S]))
        ins, seg = C.host_maps(ann, ds.image_ids[i], (rh, rw), flip, (oh, ow), S)
        inss.append(ins)
        segs.append(seg)
    im = torch.from_numpy(np.stack(ims)).cuda()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    want_x = (im.float() / 255.0 - mean) / std
    ins, seg = np.stack(inss), np.stack(segs)
    if augment:
        want_x = affine_nearest(want_x, mats)
        warp = lambda maps: affine_nearest(torch.from_numpy(maps).cuda().float().unsqueeze(1), mats).squeeze(1).round().long() \
            .cpu().numpy()                                    # noqa: E731
        ins, seg = warp(ins), warp(seg)
    assert x.shape == (3, 3, S, S) and torch.equal(x, want_x)
    assert y_mask.shape == (3, T, S * S)
    classes = set()
    for b in range(3):
        t = sequence_from_masks(ins[b], seg[b], T)
        assert np.array_equal(y_mask[b].cpu().numpy(), t[:, :-3].astype(np.float32))
        assert np.array_equal(y_class[b].cpu().numpy(), t[:, -3].astype(np.int64))
        assert np.array_equal(sw_mask[b].cpu().numpy(), t[:, -2].astype(np.float32))
        assert np.array_equal(sw_class[b].cpu().numpy(), t[:, -1].astype(np.float32))
        assert sw_mask[b].sum() >= 3
        classes |= set(y_class[b].cpu().numpy().tolist()) - {0}
    assert classes == {1, 2, 3}
    # a second epoch (decode cache, the other pinned set) gives the same batch for the same draws
    if not augment:
        dl2 = DeviceLoader(ds, 3, shuffle=False, num_workers=2, seed=seed)
        again = next(iter(dl2))
        assert all(torch.equal(p, q) for p, q in zip(again, (x, y_mask, y_class, sw_mask, sw_class)))


def test_train_py_runs_on_coco(coco_tree, tmp_path):
    """`train.py -dataset coco`: two iterations, small, end to end on the device, finite losses"""
    models = str(tmp_path / "models")
    cmd = [sys.executable, "-m", "rsis_amd.train", "-dataset", "coco", "-coco_dir", coco_tree, "-num_classes", "4", "-imsize", "64",
           "-batch_size", "2", "-maxseqlen", "3", "-gt_maxseqlen", "20", "-max_epoch", "1", "-hidden_size", "32", "--augment", "--resize",
           "--log_term", "-model_name", "coco_smoke", "-models_root", models, "-num_workers", "2", "-print_every", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"(?:total|class|iou|stop):(\S+)", r.stdout)]
    assert "Epoch 0:" in r.stdout and len(re.findall(r"^iter \d+:", r.stdout, flags=re.M)) >= 2
    assert len(losses) >= 8 and np.isfinite(losses).all() and "nan" not in r.stdout.lower()
    assert os.path.exists(os.path.join(models, "coco_smoke", "encoder.pt"))


def test_eval_py_writes_a_coco_results_file_that_the_command_line_scores_the_same(coco_tree, tmp_path, monkeypatch):
    """eval.py -dataset coco on the val split with a stand-in network that predicts every image's own instances at the input size:
    the results file carries the file's image ids and ORIGINAL category ids, and `python -m rsis_amd.cocoeval` on the annotation file
    and that results file reproduces the in-process stats exactly"""
    from rsis_amd import cocoeval as CE
    from rsis_amd import eval as EV
    from rsis_amd.args import get_parser
    ann_path = os.path.join(coco_tree, "annotations", "instances_val2017.json")
    ann = _annotation(coco_tree, "val2017")
    a = get_parser().parse_args(["-dataset", "coco", "-coco_dir", coco_tree, "-eval_split", "val", "-batch_size", "2", "-imsize", "64",
                                 "--resize", "-maxseqlen", "8", "-num_classes", "4", "-hidden_size", "32", "-model_name", "coco_eval",
                                 "-num_workers", "2", "-min_size", "0", "--display"])
    a.models_root = str(tmp_path / "models")
    torch.manual_seed(0)
    ev = EV.Evaluate(a)
    assert ev.sample_list == [im["id"] for im in ann["images"][:4]] and ev.category_ids == [0, 3, 17, 44]
    seen = []

    def fake(args, encoder, decoder, x, return_logits=False):
        k0, B, T = sum(seen), x.shape[0], args.maxseqlen
        seen.append(B)
        out, cls = torch.zeros((B, T, 64, 64)), torch.zeros((B, T, 4))
        for s in range(B):
            ins, seg = C.host_maps(ann, ev.sample_list[k0 + s], (64, 64))
            for t, k in enumerate(int(v) for v in np.unique(ins) if v > 0):
                out[s, t] = torch.from_numpy((ins == k).astype(np.float32))
                cls[s, t, int(seg[ins == k][0])] = 1.0
        return out.cuda(), cls.cuda(), torch.ones((B, T, 1)).cuda()

    monkeypatch.setattr("rsis_amd.eval_common.test", fake)
    preds = ev.run_eval()
    assert seen == [2, 2] and len(preds) > 0
    figs = os.path.join(a.models_root, "coco_eval", "coco_eval_figs_val")       # --display: the images come through image_path
    assert sorted(os.listdir(figs)) == sorted("%d.png" % i for i in ev.sample_list) and all(len(f[1]) > 0 for f in ev.figures)
    path = os.path.join(a.models_root, "coco_eval", "coco_eval_val_predictions.json")
    with open(path) as f:
        recs = json.load(f)
    names = {c["id"]: c["name"] for c in ann["categories"]}
    assert {r["image_id"] for r in recs} == set(ev.sample_list) and all(isinstance(r["image_id"], int) for r in recs)
    assert {r["category_id"] for r in recs} == {3, 17, 44} and all(r["category_name"] == names[r["category_id"]] for r in recs)
    sizes = {im["id"]: [im["height"], im["width"]] for im in ann["images"]}
    assert all(r["segmentation"]["size"] == sizes[r["image_id"]] and isinstance(r["segmentation"]["counts"], str) for r in recs)
    out = str(tmp_path / "cli.json")
    res = CE.main(["--gt", ann_path, "--dt", path, "--out", out])
    print("stats:", ev.coco_stats["stats"])
    assert res["stats"] == ev.coco_stats["stats"] and res["per_class"] == ev.coco_stats["per_class"]
    # (the file's own instances, resampled: ids that did not line up between reader, writer and scorer would give exactly 0 or -1)
    assert ev.coco_stats["stats"][0] > 0 and ev.coco_stats["stats"][1] > 0
    assert ev.coco_stats["params"]["catIds"] == [3, 17, 44] and ev.coco_stats["params"]["images"] == 5
