"""Pascal VOC on the device: the grouped target kernel (rsis_targets_from_maps) against sequence_from_masks, the two preparation
kernels (rsis_palette_to_ids, rsis_idmap_rle_encode) against numpy / rsis_rle_encode, `python -m rsis_amd.pascal_precompute` on a
synthesized tree, the DeviceLoader on a dataset with a class map of its own, and train.py / eval.py with `-dataset pascal`.
Every comparison is exact: the kernels work on integers."""
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_pascal_host import _args, decode, precompute_tree_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(5, 7), (37, 53), (96, 112)]                  # (96 x 112: more than one block per image in both launches)


def _scatter(r, H, W, ids):
    """an (H, W) map holding every id of `ids`, with DISTINCT areas (1, 2, 3, ... units, the last id takes the rest), scattered"""
    k, hw = len(ids), H * W
    unit = hw // (k * (k + 1) // 2)
    assert unit >= 1
    sizes = [unit * (j + 1) for j in range(k)]
    sizes[-1] += hw - sum(sizes)
    return np.repeat(np.asarray(ids, np.int64), sizes)[r.permutation(hw)].reshape(H, W)


def _images(H, W):
    """name -> (ins, seg): the cases of the issue at one size"""
    r = np.random.default_rng(H * 1000 + W)
    out = {}
    ins = _scatter(r, H, W, [0, 1, 2, 3, 4, 5, 6])
    out["six"] = (ins, (ins * 3 + 1) % 21)                                   # 6 instances, one class each
    ins = _scatter(r, H, W, [0, 17, 9])
    out["two"] = (ins, np.where(ins > 0, 15, 0))
    out["one_id"] = (np.full((H, W), 7, np.int64), r.integers(0, 21, (H, W)))   # no instance at all: sw_class[0] = 1
    ins = _scatter(r, H, W, [200, 3, 255])
    out["no_zero"] = (ins, r.integers(1, 21, (H, W)))                        # the smallest id present (3) is the background
    flat = np.zeros(H * W, np.int64)                                         # ids 4 and 9 of EQUAL area, id 12 over two classes
    q = H * W // 5
    flat[0:q], flat[q:2 * q], flat[2 * q:3 * q + 1] = 4, 9, 12
    seg = np.zeros(H * W, np.int64)
    seg[0:q], seg[q:2 * q], seg[2 * q:3 * q + 1] = 8, 2, 5
    seg[3 * q] = 3                                                           # one pixel of instance 12 has the smaller class
    p = r.permutation(H * W)
    out["ties"] = (flat[p].reshape(H, W), seg[p].reshape(H, W))
    return out


_CASES = {}


def _case(size, batch, T):
    """(ins (3, H, W), seg, reference tensors) -- the reference (sequence_from_masks, numpy) is computed once per case"""
    from rsis_amd.dataloader import sequence_from_masks
    key = (size, batch, T)
    if key not in _CASES:
        imgs = _images(*size)
        names = {"a": ("six", "no_zero", "ties"), "b": ("two", "one_id", "ties")}[batch]
        ins = np.stack([imgs[n][0] for n in names])
        seg = np.stack([imgs[n][1] for n in names])
        t = np.stack([sequence_from_masks(i, s, T) for i, s in zip(ins, seg)])
        ref = (t[:, :, :-3].astype(np.float32), t[:, :, -3].astype(np.int64), t[:, :, -2].astype(np.float32), t[:, :, -1].astype(np.float32))
        _CASES[key] = (ins, seg, ref)
    return _CASES[key]


def _equal(got, ref):
    for g, w in zip(got, ref):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [4, 20])
@pytest.mark.parametrize("batch", ["a", "b"])
@pytest.mark.parametrize("size", SIZES, ids=["5x7", "37x53", "96x112"])
def test_targets_kernel_equals_sequence_from_masks(size, batch, T):
    from rsis_amd.dataloader.targets import targets_from_maps, targets_kernel
    ins, seg, ref = _case(size, batch, T)
    if batch == "a":                                          # the cases are what they claim to be
        assert len(np.unique(ins[0])) - 1 == 6 and 0 not in ins[1] and set(np.unique(ins[1])) == {3, 200, 255}
    else:
        assert len(np.unique(ins[0])) - 1 == 2 and len(np.unique(ins[1])) == 1 and ref[3][1, 0] == 1 and ref[2][1].sum() == 0
    assert (ins[2] == 4).sum() == (ins[2] == 9).sum() and len(np.unique(seg[2][ins[2] == 12])) == 2
    d_ins, d_seg = torch.from_numpy(ins).cuda(), torch.from_numpy(seg).cuda()
    got = targets_kernel(d_ins, d_seg, T)
    assert got is not None, "the kernel refused ids within 0..255"
    _equal(got, ref)
    # the kernel writes every element itself: the same call over buffers the allocator hands back dirty
    junk = torch.full((3, T, size[0] * size[1]), 7.0, device="cuda")
    del junk
    _equal(targets_kernel(d_ins, d_seg, T), ref)
    # the public wrapper, and the per-image loop it keeps as fallback: bit-equal
    _equal(targets_from_maps(d_ins, d_seg, T), ref)
    loop = targets_from_maps(d_ins, d_seg, T, use_kernel=False)
    for g, w in zip(got, loop):
        assert g.dtype == w.dtype and torch.equal(g, w)


@pytest.mark.gpu
def test_targets_kernel_refuses_ids_above_255_and_the_wrapper_falls_back():
    from rsis_amd._lib import lib, ptr, stream
    from rsis_amd.dataloader import sequence_from_masks
    from rsis_amd.dataloader.targets import ERR_UNSUPPORTED, targets_from_maps, targets_kernel
    ins, seg, _ = _case((37, 53), "a", 4)
    ins = ins.copy()
    ins[0][ins[0] == 6] = 256
    d_ins, d_seg = torch.from_numpy(ins).cuda(), torch.from_numpy(seg).cuda()
    B, H, W, T = 3, 37, 53, 4
    L = lib()
    i32, s32 = d_ins.to(torch.int32), d_seg.to(torch.int32)
    ym = torch.empty((B, T, H * W), device="cuda")
    yc = torch.empty((B, T), dtype=torch.int64, device="cuda")
    sm, sc = torch.empty((B, T), device="cuda"), torch.empty((B, T), device="cuda")
    work = torch.empty((int(L.rsis_targets_work_ints(B)),), dtype=torch.int32, device="cuda")
    assert work.numel() >= 2 * 256 * B + 1
    rc = L.rsis_targets_from_maps(ptr(i32), ptr(s32), B, H, W, T, ptr(ym), ptr(yc), ptr(sm), ptr(sc), ptr(work), stream())
    assert rc == ERR_UNSUPPORTED == 3
    assert targets_kernel(d_ins, d_seg, T) is None
    t = np.stack([sequence_from_masks(i, s, T) for i, s in zip(ins, seg)])
    _equal(targets_from_maps(d_ins, d_seg, T),
           (t[:, :, :-3].astype(np.float32), t[:, :, -3].astype(np.int64), t[:, :, -2].astype(np.float32), t[:, :, -1].astype(np.float32)))


@pytest.mark.gpu
def test_palette_to_ids_equals_numpy():
    from rsis_amd.dataloader.pascal import palette_table
    from rsis_amd.pascal_precompute import ids_from_colors_numpy, palette_to_ids
    r = np.random.default_rng(3)
    voc = palette_table()
    big = np.concatenate([r.integers(0, 256, (255, 4)), [[9, 9, 9, 77]]]).astype(np.uint8)
    big[200, :3] = big[10, :3]                                # a colour listed twice: the FIRST entry wins
    big[200, 3] = big[10, 3] ^ 1
    for table in (voc, big):
        rgb = r.integers(0, 256, (37, 53, 3)).astype(np.uint8)                # colours outside the table ...
        pick = r.random((37, 53)) < 0.6
        rgb[pick] = table[r.integers(0, len(table), int(pick.sum())), :3]     # ... and rows of it
        rgb[0, 0], rgb[36, 52] = table[-1, :3], table[0, :3]
        want = ids_from_colors_numpy(rgb, table)
        assert len(np.unique(want)) > 10
        got = palette_to_ids(torch.from_numpy(rgb).cuda(), torch.from_numpy(table).cuda())
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


def _rle_encode_masks(masks):
    """rsis_rle_encode of (k, len) CUDA uint8 masks -> list of uint32 count arrays"""
    from rsis_amd._lib import check, lib, ptr, stream
    k, ln = masks.shape
    counts = torch.empty((k, ln + 1), dtype=torch.int32, device="cuda")
    nruns = torch.empty((k,), dtype=torch.int32, device="cuda")
    check(lib().rsis_rle_encode(ptr(masks), k, ln, ptr(counts), ln + 1, ptr(nruns), stream()), "rsis_rle_encode")
    nr = nruns.cpu().numpy()
    assert (nr > 0).all()
    c = counts.cpu().numpy().view(np.uint32)
    return [c[j, :nr[j]] for j in range(k)]


@pytest.mark.gpu
def test_idmap_rle_encode_equals_rle_encode_of_the_byte_masks():
    from rsis_amd.pascal_precompute import idmap_rle_counts
    r = np.random.default_rng(4)
    h, w = 37, 53
    blocky = np.kron(r.integers(0, 6, (8, 11)), np.ones((5, 5), np.int64))[:h, :w].astype(np.uint8)   # ids 0..5 in 5 x 5 blocks
    blocky[blocky == 5] = 255
    noisy = r.integers(0, 4, (h, w)).astype(np.uint8)                       # ~ hw / 2 runs per id: far more than cap = 8
    big = np.kron(r.integers(0, 3, (20, 13)), np.ones((7, 11), np.int64)).astype(np.uint8)            # 140 x 143: more than one chunk
    for idmap, ids, cap in ((blocky, [0, 1, 255, 3, 9], None), (noisy, [2, 0, 7], 8), (big, [1, 5, 2], None)):
        assert any(i not in idmap for i in ids)                            # an id that is absent from the map: one run of zeros
        d = torch.from_numpy(idmap).cuda()
        got = idmap_rle_counts(d, ids, cap=cap)
        masks = torch.stack([(d.t().contiguous().reshape(-1) == i).to(torch.uint8) for i in ids])     # column-major byte masks
        want = _rle_encode_masks(masks)
        assert len(got) == len(want) == len(ids)
        for g, x, i in zip(got, want, ids):
            assert g.dtype == np.uint32 and np.array_equal(g, x) and int(g.sum()) == idmap.size
            if i not in idmap:
                assert g.tolist() == [idmap.size]


@pytest.fixture(scope="module")
def voc_tree(tmp_path_factory):
    """a synthesized tree of 6 images, prepared by the CLI (train) and by its main() (val); the numpy statement of its ProcMasks"""
    from rsis_amd import pascal_precompute
    from rsis_amd.dataloader.pascal import synthesize_pascal_dir
    d = synthesize_pascal_dir(str(tmp_path_factory.mktemp("voc") / "VOC"), n=6, sizes=((48, 64), (75, 50)), seed=6)
    truth = precompute_tree_numpy(d)
    for f in os.listdir(os.path.join(d, "ProcMasks")):      # (the numpy statement wrote them: the preparation under test starts from none)
        os.unlink(os.path.join(d, "ProcMasks", f))
    r = subprocess.run([sys.executable, "-m", "rsis_amd.pascal_precompute", "--pascal_dir", d, "--split", "train"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    pascal_precompute.main(["--pascal_dir", d, "--split", "val"])
    return d, truth


@pytest.mark.gpu
def test_precompute_cli_writes_masks_and_ground_truth(voc_tree):
    from rsis_amd import pascal_precompute
    from rsis_amd.utils.utils import load_plain_pickle
    d, truth = voc_tree
    n_rec = 0
    for split, n in (("train", 4), ("val", 2)):
        names = pascal_precompute.get_imnames(d, split)
        assert len(names) == n
        recs = load_plain_pickle(os.path.join(d, "VOCGT_%s.pkl" % split))
        assert [r["image_id"] for r in recs if r["ignore"] == 1] == [nm for nm in names for _ in range(20)]
        for nm in names:
            masks, ignore = truth[nm]
            got = np.load(os.path.join(d, "ProcMasks", nm + ".npy"))
            assert got.dtype == np.uint8 and got.shape == masks.shape and np.array_equal(got, masks)
            mine = [r for r in recs if r["image_id"] == nm]
            ids = np.unique(masks[:, :, 1])[1:]
            assert len(mine) == len(ids) + 20 and [r["ignore"] for r in mine] == [0] * len(ids) + [1] * 20
            for r, i in zip(mine, ids):                       # ascending ids; every RLE decodes to its instance mask
                assert r["segmentation"]["size"] == list(masks.shape[:2])
                assert np.array_equal(decode(r["segmentation"]), (masks[:, :, 1] == i).astype(np.uint8))
                assert r["category_id"] == int(masks[:, :, 0][masks[:, :, 1] == i].min()) and r["score"] == 1
            assert [r["category_id"] for r in mine[len(ids):]] == list(range(1, 21))
            assert all(np.array_equal(decode(r["segmentation"]), ignore) for r in mine[len(ids):])
            n_rec += len(mine)
    # a second run finds the masks, recomputes the ignore masks from the class PNGs and writes the same records
    with open(os.path.join(d, "VOCGT_val.pkl"), "rb") as f:
        before = f.read()
    again = pascal_precompute.run(d, "val", forcegen=False, verbose=False)
    with open(os.path.join(d, "VOCGT_val.pkl"), "rb") as f:
        assert f.read() == before and pickle.loads(before) == again
    assert n_rec > 6 * 22


@pytest.mark.gpu
def test_device_loader_on_pascal_targets_equal_sequence_from_masks_of_the_warped_maps(voc_tree):
    """augmentation on, three classes: image, instance map and class map share one warp per sample, and the targets are exactly
    sequence_from_masks of the warped maps"""
    from rsis_amd.dataloader import sequence_from_masks
    from rsis_amd.dataloader.augment import affine_nearest
    from rsis_amd.dataloader.loader import MEAN, STD, DeviceLoader
    from rsis_amd.dataloader.pascal import PascalVOC
    d, _ = voc_tree
    S, T = 32, 10
    ds = PascalVOC(_args(d, batch_size=3), split="train", imsize=S, augment=True)
    dl = DeviceLoader(ds, 3, shuffle=False, num_workers=2, seed=5)
    assert len(dl) == 1
    random.seed(11)                                           # RandomAffine draws from python's global stream, as the reference does
    x, y_mask, y_class, sw_mask, sw_class = next(iter(dl))
    rng = random.Random(5 * 1000003 + 1)                      # the loader's per-sample stream of rank 0
    seeds = [rng.getrandbits(32) for _ in range(3)]
    host = [ds.host_item(i, random.Random(s)) for i, s in zip(range(3), seeds)]
    random.seed(11)
    mats = torch.stack([ds.augmentation_transform.matrix(S, S) for _ in range(3)])
    im = torch.from_numpy(np.stack([h[0] for h in host])).cuda()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    assert torch.equal(x, affine_nearest((im.float() / 255.0 - mean) / std, mats))
    warp = lambda k: affine_nearest(torch.from_numpy(np.stack([h[k] for h in host])).cuda().float().unsqueeze(1), mats) \
        .squeeze(1).round().long().cpu().numpy()              # noqa: E731
    ins, seg = warp(1), warp(2)
    assert x.shape == (3, 3, S, S) and y_mask.shape == (3, T, S * S)
    assert len(set(np.unique(seg).tolist()) - {0}) == 3 and any(not np.array_equal(ins[b], host[b][1]) for b in range(3))
    for b in range(3):
        t = sequence_from_masks(ins[b], seg[b], T)
        assert np.array_equal(y_mask[b].cpu().numpy(), t[:, :-3].astype(np.float32))
        assert np.array_equal(y_class[b].cpu().numpy(), t[:, -3].astype(np.int64))
        assert np.array_equal(sw_mask[b].cpu().numpy(), t[:, -2].astype(np.float32))
        assert np.array_equal(sw_class[b].cpu().numpy(), t[:, -1].astype(np.float32))
        assert set(y_class[b].cpu().numpy().tolist()) - {0} <= {2, 7, 15} and sw_mask[b].sum() >= 1


@pytest.mark.gpu
def test_train_py_runs_on_pascal(voc_tree, tmp_path):
    """`train.py -dataset pascal --resize` (the flag set of the reference's train_pascal.sh, small) end to end on the device"""
    d, _ = voc_tree
    models = str(tmp_path / "models")
    cmd = [sys.executable, "-m", "rsis_amd.train", "-dataset", "pascal", "--resize", "-imsize", "64", "-batch_size", "2", "-maxseqlen", "3",
           "-max_epoch", "1", "--log_term", "-pascal_dir", d, "-model_name", "pascal_smoke", "-models_root", models, "-num_workers", "2",
           "-hidden_size", "32", "-print_every", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Epoch 0:" in r.stdout and "nan" not in r.stdout.lower()
    assert os.path.exists(os.path.join(models, "pascal_smoke", "encoder.pt"))


@pytest.mark.gpu
def test_eval_py_scores_the_ground_truth_of_pascal_as_perfect(tmp_path, monkeypatch):
    """eval.py -dataset pascal with a stand-in network that predicts every image's own ground-truth instances (stop 1, one-hot class):
    originals of 64 x 80 at -imsize 64 are not resized, so AP must be exactly 1 -- any slip in ids, categories, sizes, element order
    or ignore pixels between the preparation, the reader and the evaluator lowers it"""
    from rsis_amd import pascal_precompute
    from rsis_amd.args import get_parser
    from rsis_amd.dataloader.pascal import synthesize_pascal_dir
    from rsis_amd.eval import Evaluate
    d = synthesize_pascal_dir(str(tmp_path / "VOC"), n=5, sizes=((64, 80),), seed=8)
    pascal_precompute.run(d, "val", verbose=False)
    before = sorted(os.listdir(d))
    a = get_parser().parse_args(["-dataset", "pascal", "-pascal_dir", d, "-eval_split", "val", "-batch_size", "1", "-imsize", "64",
                                 "-maxseqlen", "8", "-hidden_size", "32", "-model_name", "pascal_eval", "-num_workers", "2"])
    a.models_root = str(tmp_path / "models")
    torch.manual_seed(0)
    ev = Evaluate(a)
    names = pascal_precompute.get_imnames(d, "val")
    assert ev.sample_list == names and len(names) == 2 and len(ev.class_names) == 21
    seen = []

    def fake(args, encoder, decoder, x, return_logits=False):
        k = len(seen)
        seen.append(tuple(x.shape))
        masks = np.load(os.path.join(d, "ProcMasks", names[k] + ".npy"))
        seg, ins = masks[:, :, 0], masks[:, :, 1]
        T = args.maxseqlen
        out = torch.zeros((1, T) + ins.shape)
        cls = torch.zeros((1, T, 21))
        for t, i in enumerate(np.unique(ins)[1:]):
            out[0, t] = torch.from_numpy((ins == i).astype(np.float32))
            cls[0, t, int(seg[ins == i].min())] = 1.0
        return out.cuda(), cls.cuda(), torch.ones((1, T, 1)).cuda()

    monkeypatch.setattr("rsis_amd.eval_common.test", fake)
    preds = ev.run_eval()
    assert seen == [(1, 3, 64, 80)] * 2                        # un-cropped, un-resized, in sample order
    assert preds and all(p["segmentation"]["size"] == [64, 80] for p in preds)
    assert ev.coco_stats["stats"][0] == 1.0, ev.coco_stats["stats"]
    assert sorted(os.listdir(d)) == before                     # nothing is written into the dataset directory
