"""Cityscapes on the device: rsis_instance_maps against its numpy statement (tests/cityscapes_reader_cases.py), the targets of its maps
against sequence_from_masks of the reference's full procedure, the DeviceLoader on a synthesized tree, `train.py -dataset cityscapes`
and `eval_cityscapes` on real files.  Every comparison is exact: the kernels work on integers."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cityscapes_reader_cases as C  # noqa: E402
from test_cityscapes_reader_host import _args  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(5, 7), (37, 53), (96, 112)]                  # (96 x 112: more than one block per image in both launches)
SIZE_IDS = ["5x7", "37x53", "96x112"]
NAMES = ["mixed", "none", "no_background", "custom", "dense"]

_CASES = {}


def _case(size, name):
    """(raw (3, H, W), table, (ins, seg) by the numpy statement) -- computed once per case"""
    key = (size, name)
    if key not in _CASES:
        raw = C.device_cases(*size)[name]
        table = C.CUSTOM_TABLE if name == "custom" else C.TABLE
        _CASES[key] = (raw, table, C.device_rule(raw, table))
    return _CASES[key]


def _params(names):
    """(size, name) of every case that exists: `dense` (300 ids) at 96 x 112 only"""
    return [pytest.param(size, name, id="%s-%s" % (sid, name)) for size, sid in zip(SIZES, SIZE_IDS) for name in names
            if name != "dense" or size == (96, 112)]


def _call(raw_d, tab_d, ins, seg, work):
    from rsis_amd._lib import check, lib, ptr, stream
    B, H, W = raw_d.shape
    check(lib().rsis_instance_maps(ptr(raw_d), ptr(tab_d), int(tab_d.numel()), B, H, W, ptr(ins), ptr(seg), ptr(work), stream()),
          "rsis_instance_maps")


@pytest.mark.gpu
@pytest.mark.parametrize("size,name", _params(NAMES))
def test_instance_maps_equal_the_numpy_statement(size, name):
    from rsis_amd._lib import lib
    from rsis_amd.dataloader.cityscapes import maps_from_ids
    raw, table, (want_ins, want_seg) = _case(size, name)
    # the cases are what they claim to be
    if name == "mixed":
        assert set(C.MIXED_VALUES) <= set(raw[0].reshape(-1).tolist()) and {24000, 24999, 33999, 5000, 34000, 65535, -1, 70000} <= set(C.MIXED_VALUES)
        assert want_ins[0].max() == 16 and (want_seg[0][raw[0] // 1000 == 29] == 0).all() and (want_ins[0][raw[0] == 65535] == 0).all()
    elif name == "none":
        assert not want_ins.any() and not want_seg.any()
    elif name == "no_background":
        assert (want_ins > 0).all() and want_ins[0].max() == 24 and want_ins[1].max() == 1
    elif name == "custom":
        assert want_seg[0][raw[0] == 1000].tolist()[0] == 3 and want_seg[0][raw[0] == 65535].tolist()[0] == 2
        assert want_ins[0][raw[0] == 1000].tolist()[0] == 1 and want_ins[0].max() == 4 and (want_ins[0][raw[0] == 24000] == 0).all()
        assert want_ins[0][raw[0] == 65535].tolist()[0] == 4
    else:
        assert want_ins[0].max() == 300 and want_ins[1].max() == 256 and want_ins[2].max() == 255
    raw_d = torch.from_numpy(raw).cuda()
    tab_d = torch.tensor(table, dtype=torch.int32, device="cuda")
    ins, seg = maps_from_ids(raw_d, None if name != "custom" else tab_d)
    assert ins.dtype == seg.dtype == torch.int32 and ins.shape == seg.shape == raw_d.shape
    assert np.array_equal(ins.cpu().numpy(), want_ins) and np.array_equal(seg.cpu().numpy(), want_seg)
    ins64, seg64 = maps_from_ids(raw_d.long(), None if name != "custom" else tab_d)       # (what the loader passes: int64)
    assert torch.equal(ins64, ins) and torch.equal(seg64, seg)
    # the same call into dirty output buffers and dirty scratch: every element is written, the scratch is zeroed by the call
    B = raw.shape[0]
    n_work = int(lib().rsis_instance_maps_work_ints(B))
    assert n_work >= 2048 * B
    ins2, seg2 = torch.full_like(raw_d, -77), torch.full_like(raw_d, 12345)
    work = torch.full((n_work,), -1, dtype=torch.int32, device="cuda")
    _call(raw_d, tab_d, ins2, seg2, work)
    assert torch.equal(ins2, ins) and torch.equal(seg2, seg)
    _call(raw_d, tab_d, ins2, seg2, work)                      # and again over the scratch the first call left
    assert torch.equal(ins2, ins) and torch.equal(seg2, seg)


@pytest.mark.gpu
def test_instance_maps_refuses_bad_arguments():
    from rsis_amd._lib import lib, ptr, stream
    L = lib()
    raw = torch.zeros((1, 4, 4), dtype=torch.int32, device="cuda")
    ins, seg = torch.empty_like(raw), torch.empty_like(raw)
    tab = torch.zeros((67,), dtype=torch.int32, device="cuda")
    work = torch.empty((2048,), dtype=torch.int32, device="cuda")
    assert L.rsis_instance_maps_work_ints(0) == 0 and L.rsis_instance_maps_work_ints(32) == 32 * 2048
    assert L.rsis_instance_maps(ptr(raw), ptr(tab), 67, 1, 4, 4, ptr(ins), ptr(seg), ptr(work), stream()) == 1
    assert L.rsis_instance_maps(ptr(raw), ptr(tab), 0, 1, 4, 4, ptr(ins), ptr(seg), ptr(work), stream()) == 1
    assert L.rsis_instance_maps(ptr(raw), ptr(tab), 34, 1, 4, 4, ptr(raw), ptr(seg), ptr(work), stream()) == 1
    assert L.rsis_instance_maps(ptr(raw), None, 34, 1, 4, 4, ptr(ins), ptr(seg), ptr(work), stream()) == 1
    assert L.rsis_instance_maps(ptr(raw), ptr(tab), 34, 1, 4, 4, ptr(ins), ptr(seg), ptr(work), stream()) == 0


def _as_targets(t):
    return (t[:, :, :-3].astype(np.float32), t[:, :, -3].astype(np.int64), t[:, :, -2].astype(np.float32), t[:, :, -1].astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [4, 20])
@pytest.mark.parametrize("size,name", _params(["mixed", "none", "dense"]))
def test_targets_of_the_kernels_maps_equal_sequence_from_masks_of_the_reference_maps(size, name, T):
    """reference maps: the reference's full procedure (reference_raw_sample) on the ids with the values it is not defined for -- outside
    0..65535, or >= 1000 with a label outside 24..33 -- set to 0"""
    from rsis_amd.dataloader import sequence_from_masks
    from rsis_amd.dataloader.cityscapes import maps_from_ids
    from rsis_amd.dataloader.targets import targets_from_maps, targets_kernel
    raw, _table, _maps = _case(size, name)
    key = (size, name, T)
    if key not in _CASES:
        ref = [C.reference_raw_sample(C.defined_for_reference(r)) for r in raw]
        _CASES[key] = _as_targets(np.stack([sequence_from_masks(i, s, T) for i, s in ref]))
    want = _CASES[key]
    ins, seg = maps_from_ids(torch.from_numpy(raw).cuda())
    grouped = targets_kernel(ins, seg, T)
    if name == "dense":
        assert grouped is None                                 # ranks above 255: the grouped kernel refuses, the wrapper falls back
    else:
        assert grouped is not None
    got = targets_from_maps(ins, seg, T)
    for g, w in zip(got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    if name == "none":
        assert (got[3][:, 0] == 1).all() and not got[2].any() and not got[0].any()
    if name == "mixed":
        assert (got[2][0].sum() == min(T, 16)) and set(got[1].cpu().numpy().reshape(-1).tolist()) <= set(range(9))


@pytest.fixture(scope="module")
def city_tree(tmp_path_factory):
    from rsis_amd.dataloader.cityscapes import synthesize_cityscapes_dir
    return synthesize_cityscapes_dir(str(tmp_path_factory.mktemp("cs") / "CityScapes"), n=4, sizes=((64, 128),), seed=6)


@pytest.mark.gpu
def test_device_loader_on_cityscapes_targets_equal_sequence_from_masks_of_the_warped_reference_maps(city_tree):
    """augmentation on, batch 3 of un-cropped 32 x 64 samples: x is the normalised, warped PIL resize; the targets are exactly
    sequence_from_masks of the reference's maps (full-resolution procedure -> zoom of both -> flip -> the same warp)"""
    from PIL import Image
    from rsis_amd.dataloader import sequence_from_masks, targets
    from rsis_amd.dataloader.augment import affine_nearest
    from rsis_amd.dataloader.cityscapes import CityScapes
    from rsis_amd.dataloader.loader import MEAN, STD, DeviceLoader
    S, T = (32, 64), 20
    ds = CityScapes(_args(city_tree), split="train", imsize=32, augment=True)
    dl = DeviceLoader(ds, 3, shuffle=False, num_workers=2, seed=5)
    assert len(dl) == 1 and ds.crop is False
    calls = []
    real = targets.targets_kernel

    def spy(ins, seg, max_seq_len):
        out = real(ins, seg, max_seq_len)
        calls.append(out is not None)
        return out
    targets.targets_kernel = spy
    try:
        random.seed(11)                                       # RandomAffine draws from python's global stream, as the reference does
        x, y_mask, y_class, sw_mask, sw_class = next(iter(dl))
    finally:
        targets.targets_kernel = real
    assert calls == [True]                                    # the batch took the grouped kernel: one host sync
    rng = random.Random(5 * 1000003 + 1)                      # the loader's per-sample stream of rank 0
    seeds = [rng.getrandbits(32) for _ in range(3)]
    flips = [random.Random(s).random() < 0.5 for s in seeds]  # host_item's first draw
    random.seed(11)
    mats = torch.stack([ds.augmentation_transform.matrix(S[0], S[1]) for _ in range(3)])
    ims, inss, segs = [], [], []
    for i, f in enumerate(flips):
        with Image.open(ds.image_files[i]) as im:
            a = np.asarray(im.convert("RGB").resize((S[1], S[0]), Image.BILINEAR)).transpose(2, 0, 1)
        ins, seg = C.reference_raw_sample(ds.raw_ids(i))
        ins, seg = C.zoom_nearest(ins, S), C.zoom_nearest(seg, S)
        if f:
            a, ins, seg = a[:, :, ::-1], ins[:, ::-1], seg[:, ::-1]
        ims.append(np.ascontiguousarray(a))
        inss.append(np.ascontiguousarray(ins))
        segs.append(np.ascontiguousarray(seg))
    im = torch.from_numpy(np.stack(ims)).cuda()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    assert x.shape == (3, 3, 32, 64) and torch.equal(x, affine_nearest((im.float() / 255.0 - mean) / std, mats))
    warp = lambda maps: affine_nearest(torch.from_numpy(np.stack(maps)).cuda().float().unsqueeze(1), mats) \
        .squeeze(1).round().long().cpu().numpy()              # noqa: E731
    ins, seg = warp(inss), warp(segs)
    assert y_mask.shape == (3, T, 32 * 64) and any(not np.array_equal(ins[b], inss[b]) for b in range(3))
    classes = set()
    for b in range(3):
        t = sequence_from_masks(ins[b], seg[b], T)
        assert np.array_equal(y_mask[b].cpu().numpy(), t[:, :-3].astype(np.float32))
        assert np.array_equal(y_class[b].cpu().numpy(), t[:, -3].astype(np.int64))
        assert np.array_equal(sw_mask[b].cpu().numpy(), t[:, -2].astype(np.float32))
        assert np.array_equal(sw_class[b].cpu().numpy(), t[:, -1].astype(np.float32))
        assert sw_mask[b].sum() >= 2
        classes |= set(y_class[b].cpu().numpy().tolist()) - {0}
    assert classes and classes <= set(range(1, 9))


@pytest.mark.gpu
def test_train_py_runs_on_cityscapes(city_tree, tmp_path):
    """`train.py -dataset cityscapes` with the flag set of the reference's train_cityscapes.sh, small, end to end on the device"""
    models = str(tmp_path / "models")
    cmd = [sys.executable, "-m", "rsis_amd.train", "-dataset", "cityscapes", "-cityscapes_dir", city_tree, "-num_classes", "9", "-imsize", "32",
           "-batch_size", "2", "-maxseqlen", "3", "-gt_maxseqlen", "20", "-max_epoch", "1", "-hidden_size", "32", "--augment",
           "--curriculum_learning", "-min_steps", "1", "--log_term", "-model_name", "city_smoke", "-models_root", models, "-num_workers", "2",
           "-print_every", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Epoch 0:" in r.stdout and "nan" not in r.stdout.lower()
    assert os.path.exists(os.path.join(models, "city_smoke", "encoder.pt"))


def _listing(d):
    return sorted(os.path.join(p, f) for p, _dirs, files in os.walk(d) for f in files)


@pytest.mark.gpu
def test_eval_cityscapes_scores_the_ground_truth_of_real_files_as_perfect(city_tree, tmp_path, monkeypatch):
    """eval_cityscapes on files with a stand-in network that predicts every image's own ground-truth instances (stop 1, one-hot class):
    originals of 64 x 128 at -imsize 64 are not resized, so AP and AP50% of every class present must be exactly 1 -- any slip in file
    pairing, sample order, sizes or class ids between the reader, the writer and the scorer lowers it"""
    from rsis_amd import cityscapes_eval as E, eval_cityscapes
    from rsis_amd.args import get_parser
    before = _listing(city_tree)
    a = get_parser().parse_args(["-cityscapes_dir", city_tree, "-eval_split", "val", "-batch_size", "2", "-imsize", "64", "-maxseqlen", "10",
                                 "-num_classes", "9", "-hidden_size", "32", "-model_name", "city_eval", "-num_workers", "2"])
    a.models_root = str(tmp_path / "models")
    torch.manual_seed(0)
    ev = eval_cityscapes.Evaluate(a)
    files = ev.dataset.get_sample_list()
    assert len(files) == 4 and ev.sample_list == [os.path.basename(f)[:-len(".png")] for f in files]
    assert all(s.endswith("_leftImg8bit") for s in ev.sample_list)
    seen, present = [], set()

    def fake(args, encoder, decoder, x, return_logits=False):
        k0, B, T = sum(s[0] for s in seen), x.shape[0], args.maxseqlen
        seen.append(tuple(x.shape))
        out, cls = torch.zeros((B, T, 64, 128)), torch.zeros((B, T, 9))
        for s in range(B):
            raw = E.read_gt_png(ev.dataset.ins_files[k0 + s]).astype(np.int64)
            ids = [int(v) for v in np.unique(raw) if v >= 1000 and C.TABLE[v // 1000] > 0]
            assert 2 <= len(ids) <= T
            for t, v in enumerate(ids):
                m = raw == v
                assert m.sum() >= E.MIN_REGION                 # (and connected: synthesize_cityscapes_dir)
                out[s, t] = torch.from_numpy(m.astype(np.float32))
                cls[s, t, C.TABLE[v // 1000]] = 1.0
                present.add(v // 1000)
        return out.cuda(), cls.cuda(), torch.ones((B, T, 1)).cuda()

    monkeypatch.setattr("rsis_amd.eval_common.test", fake)
    n_lines = ev.create_figures()
    assert seen == [(2, 3, 64, 128)] * 2 and n_lines == 4 * 10 * 8   # un-cropped, un-resized, in sample order
    res = ev.score()
    assert res["images"] == 4 and len(present) >= 4
    for ci, cid in enumerate(E.CLASS_IDS):
        if cid in present:
            assert (res["aps"][ci] == 1.0).all(), (cid, res["aps"][ci])
            assert res["averages"]["classes"][E.CLASS_NAMES[ci]] == {"ap": 1.0, "ap50%": 1.0}
        else:
            assert np.isnan(res["aps"][ci]).all()
    assert res["averages"]["allAp"] == 1.0 and res["averages"]["allAp50%"] == 1.0
    results = os.path.join(a.models_root, "city_eval", "city_eval_results")
    assert sorted(f for f in os.listdir(results) if f.endswith(".txt")) == sorted(s + ".txt" for s in ev.sample_list)
    assert not os.path.exists(os.path.join(a.models_root, "city_eval", "city_eval_gt"))
    assert _listing(city_tree) == before                       # nothing is written into the dataset directory


@pytest.fixture(scope="module")
def odd_tree(tmp_path_factory):
    """three images per split: at batch 2 the last batch is one image"""
    from rsis_amd.dataloader.cityscapes import synthesize_cityscapes_dir
    return synthesize_cityscapes_dir(str(tmp_path_factory.mktemp("cs3") / "CityScapes"), n=3, sizes=((64, 128),))


def _recording_network(seen, twins, num_classes):
    """stand-in for test() that records the shape of every batch it is given (`seen`) and whether its last two images are equal
    (`twins`).  Every mask is one rectangle, every stop probability 1 and the score of class 1 is (k + 1) / 8 for the k-th image it has
    been given (exact in float32), so that an output can be traced to its input."""
    def fake(args, encoder, decoder, x, return_logits=False):
        k0, B, T = sum(s[0] for s in seen), x.shape[0], args.maxseqlen
        seen.append(tuple(x.shape))
        twins.append(B >= 2 and bool((x[-1] == x[-2]).all()))
        out = torch.zeros((B, T) + tuple(x.shape[-2:]))
        out[:, :, 8:40, 16:56] = 1.0
        cls = torch.zeros((B, T, num_classes))
        cls[:, :, 1] = (torch.arange(B) + k0 + 1).view(B, 1) / 8.0
        return out.cuda(), cls.cuda(), torch.ones((B, T, 1)).cuda()
    return fake


def _odd_args(odd_tree, tmp_path, name, *extra):
    from rsis_amd.args import get_parser
    a = get_parser().parse_args(["-cityscapes_dir", odd_tree, "-eval_split", "val", "-batch_size", "2", "-imsize", "64", "-maxseqlen", "3",
                                 "-num_classes", "9", "-hidden_size", "32", "-model_name", name, "-num_workers", "2"] + list(extra))
    a.models_root = str(tmp_path / "models")
    return a


@pytest.mark.gpu
def test_eval_cityscapes_passes_a_lone_tail_image_as_it_is(odd_tree, tmp_path, monkeypatch):
    """eval_cityscapes over 3 images at batch 2: the last batch reaches test() as ONE image (this driver does not double it), and the
    three result files hold the outputs of their own images, in sample order"""
    from rsis_amd import eval_cityscapes
    a = _odd_args(odd_tree, tmp_path, "city_tail")
    torch.manual_seed(0)
    ev = eval_cityscapes.Evaluate(a)
    seen, twins = [], []
    monkeypatch.setattr("rsis_amd.eval_common.test", _recording_network(seen, twins, 9))
    assert ev.create_figures() == 3 * 3 * 8
    assert seen == [(2, 3, 64, 128), (1, 3, 64, 128)] and twins == [False, False]
    results = os.path.join(a.models_root, "city_tail", "city_tail_results")
    assert len(ev.sample_list) == 3
    assert sorted(f for f in os.listdir(results) if f.endswith(".txt")) == sorted(s + ".txt" for s in ev.sample_list)
    for k, sample in enumerate(ev.sample_list):
        lines = open(os.path.join(results, sample + ".txt")).read().splitlines()
        assert len(lines) == 3 * 8 and all(l.startswith("city_tail_masks/%s_" % sample) for l in lines)
        assert lines[0].split()[1] == "24" and float(lines[0].split()[2]) == (k + 1) / 8.0
    assert len(ev.records) == 3


@pytest.mark.gpu
def test_eval_cityscapes_on_files_unscored_reads_no_ground_truth(odd_tree, tmp_path, monkeypatch):
    """eval_cityscapes on files under --no_run_coco_eval: the result files are written, nothing is scored, no ground-truth PNG is read
    for scoring, no `_gt` folder appears and nothing is created under the dataset tree"""
    from rsis_amd import cityscapes_eval as E, eval_cityscapes
    before = _listing(odd_tree)
    a = _odd_args(odd_tree, tmp_path, "city_unscored", "--no_run_coco_eval")
    torch.manual_seed(0)
    ev = eval_cityscapes.Evaluate(a)
    monkeypatch.setattr("rsis_amd.eval_common.test", _recording_network([], [], 9))

    def no_read(path):
        raise AssertionError("ground truth read under --no_run_coco_eval: %s" % path)

    monkeypatch.setattr(E, "read_gt_png", no_read)
    assert ev.create_figures() == 3 * 3 * 8
    assert ev.records == [] and ev.gt_dir is None and ev.score() is None
    out = os.path.join(a.models_root, "city_unscored")
    assert sorted(os.listdir(out)) == ["city_unscored_results"]
    assert _listing(odd_tree) == before


@pytest.mark.gpu
def test_eval_py_doubles_a_lone_tail_image_of_cityscapes_only(odd_tree, tmp_path, monkeypatch):
    """rsis_amd.eval -dataset cityscapes over 3 images at batch 2: the lone last image reaches test() twice and its copy's outputs are
    dropped -- records for exactly the 3 images, each with its own scores.  With --synthetic every batch goes in as the loader made it."""
    from rsis_amd.args import get_parser
    from rsis_amd.eval import Evaluate
    a = _odd_args(odd_tree, tmp_path, "city_json", "-dataset", "cityscapes", "-stop_th", "0", "-class_th", "0", "-min_size", "0")
    torch.manual_seed(0)
    ev = Evaluate(a)
    seen, twins = [], []
    monkeypatch.setattr("rsis_amd.eval_common.test", _recording_network(seen, twins, 9))
    preds = ev.run_eval()
    assert seen == [(2, 3, 64, 128), (2, 3, 64, 128)] and twins == [False, True]
    assert len(ev.sample_list) == 3 and sorted(set(p["image_id"] for p in preds)) == sorted(ev.sample_list)
    assert len(preds) == 3 * 3 * 8
    for k, sample in enumerate(ev.sample_list):
        assert {p["score"] for p in preds if p["image_id"] == sample and p["category_id"] == 1} == {(k + 1) / 8.0}
    b = get_parser().parse_args(["--synthetic", "-model_name", "syn_json", "-batch_size", "2", "-maxseqlen", "3", "-hidden_size", "32",
                                 "-synthetic_batches", "8", "-num_classes", "5", "-imsize", "64", "-stop_th", "0", "-class_th", "0",
                                 "-min_size", "0", "-models_root", str(tmp_path / "models")])
    ev = Evaluate(b)
    given = []
    inner = _recording_network(seen, twins, 5)

    def fake(args, encoder, decoder, x, return_logits=False):
        given.append(x.data_ptr())
        return inner(args, encoder, decoder, x)

    del seen[:], twins[:]
    monkeypatch.setattr("rsis_amd.eval_common.test", fake)
    assert len(ev.run_eval()) == 4 * 3 * 4
    assert seen == [(2, 3, 64, 64)] * 2 and twins == [False, False]
    assert given == [batch[0].data_ptr() for batch in ev.loader]          # the loader's own tensors, not copies
