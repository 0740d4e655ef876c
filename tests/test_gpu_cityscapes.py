"""GPU tests of the Cityscapes evaluation (rsis_amd/csrc/insteval.hip through rsis_amd/cityscapes_eval.py): the count tables are
integers and must EQUAL a numpy count table (np.unique + np.bincount; on the fixture also the golden module's boolean-image counts);
match lists equal; AP and averages within 1e-12 of the golden module (tests/test_cityscapes_host.py states where the bar comes from)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cityscapes_cases as C  # noqa: E402
import cityscapes_golden as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _same(got, gt, masks):
    want, ids = C.np_counts(gt, masks)
    assert got[1].dtype == np.int64 and np.array_equal(got[1], ids)
    assert got[0].shape == want.shape and np.array_equal(got[0], want)


def _blobs(rng, shape, n, lo=4, hi=None):
    """n rectangles (one connected component each, as the model's masks are)"""
    hi = hi or max(lo + 1, min(shape) // 2)
    out = np.zeros((n,) + tuple(shape), np.uint8)
    for k in range(n):
        h, w = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        y, x = int(rng.integers(0, shape[0] - h + 1)), int(rng.integers(0, shape[1] - w + 1))
        out[k, y:y + h, x:x + w] = 255
    return out


def _city(rng, shape, n_inst):
    gt = np.full(shape, C.ROAD, np.uint16)
    for k in range(n_inst):
        h, w = int(rng.integers(3, max(4, shape[0] // 3))), int(rng.integers(3, max(4, shape[1] // 3)))
        y, x = int(rng.integers(0, shape[0] - h + 1)), int(rng.integers(0, shape[1] - w + 1))
        gt[y:y + h, x:x + w] = int(rng.choice([24, 25, 26, 27, 28, 29, 31, 32, 33])) * 1000 + k
    return gt


def test_fixture_counts_equal_and_scores_within_the_bar():
    from rsis_amd import cityscapes_eval as E
    for case in C.load_cases():
        imgs = case["images"]
        res = E.overlap_counts_batch([i["gt"] for i in imgs], [i["masks"] for i in imgs])
        records = []
        for img, (counts, ids) in zip(imgs, res):
            assert np.array_equal(counts, img["counts"]) and np.array_equal(ids, img["ids"])
            d, di = G.direct_counts(img["gt"], img["masks"])
            assert np.array_equal(counts, d) and np.array_equal(ids, di)
        recs = E.score_image_sets([i["gt"] for i in imgs], [i["masks"] for i in imgs], [i["rows"] for i in imgs], [i["labels"] for i in imgs],
                                  [i["scores"] for i in imgs])
        for img, rec in zip(imgs, recs):
            for key in ("gt", "pred", "conf", "pairs"):
                assert np.array_equal(rec[key], img["rec_" + key]), key
            records.append(rec)
        aps = E.evaluate_matches(records)
        assert np.array_equal(np.isnan(aps), np.isnan(case["aps"]))
        print("max |AP - golden| =", np.nanmax(np.abs(aps - case["aps"])))
        assert np.nanmax(np.abs(aps - case["aps"])) <= 1e-12
        av = E.compute_averages(aps)
        assert abs(av["allAp"] - case["all"][0]) <= 1e-12 and abs(av["allAp50%"] - case["all"][1]) <= 1e-12


def test_full_size_image_with_160_masks_device_and_host_inputs():
    from rsis_amd import cityscapes_eval as E
    rng = np.random.default_rng(1)
    gt = _city(rng, (1024, 2048), 40)
    masks = _blobs(rng, (1024, 2048), 160, 20, 400)
    want = C.np_counts(gt, masks)
    got = E.overlap_counts(gt, masks)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    again = E.overlap_counts(torch.from_numpy(gt.astype(np.int32)).cuda(), torch.from_numpy(masks).cuda())   # packed by rsis_mask_pack_bits
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 130])
def test_mask_counts_around_the_group_size(P):
    from rsis_amd import cityscapes_eval as E
    rng = np.random.default_rng(100 + P)
    shape = (150, 233)                                              # 34950 pixels: three chunks, the last one partial, not a multiple of 64
    gt = _city(rng, shape, 12)
    masks = _blobs(rng, shape, P)
    _same(E.overlap_counts(gt, masks), gt, masks)


@pytest.mark.parametrize("n_ids", [300, 5000, 65535])
def test_many_distinct_ids(n_ids):
    """more ids than the LDS window holds (64), than 256 and than 4096; 65535 is the most the interface takes"""
    from rsis_amd import cityscapes_eval as E
    rng = np.random.default_rng(n_ids)
    shape = (300, 400) if n_ids < 65535 else (512, 512)
    ids = rng.choice(65536, n_ids, replace=False).astype(np.uint16)
    gt = ids[rng.integers(0, n_ids, shape)]
    gt.reshape(-1)[:n_ids] = ids                                     # every id occurs
    masks = _blobs(rng, shape, 5, 20, 150)
    got = E.overlap_counts(gt, masks)
    assert got[0].shape == (6, n_ids)
    _same(got, gt, masks)


def test_all_65536_ids_are_refused():
    from rsis_amd import cityscapes_eval as E
    gt = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    with pytest.raises(ValueError):
        E.overlap_counts(gt, np.zeros((1, 256, 256), np.uint8))


def test_images_at_odd_pool_positions_and_different_sizes_in_one_call():
    from rsis_amd import cityscapes_eval as E
    rng = np.random.default_rng(7)
    shapes = [(1, 1), (3, 5), (17, 19), (64, 64), (130, 127), (96, 160), (1, 16385), (257, 129), (5, 7)]
    gts = [_city(rng, s, 5) if min(s) > 3 else rng.integers(0, 40000, s).astype(np.uint16) for s in shapes]
    sets = [_blobs(rng, s, int(rng.integers(0, 70)), 1, max(2, min(s))) for s in shapes]
    for lead in (0, 2, 6, 14):                                       # images packed back to back after `lead` bytes: every start modulo 16
        res = E.overlap_counts_batch(gts, sets, align=2, lead=lead)
        for got, g, m in zip(res, gts, sets):
            _same(got, g, m)
    res = E.overlap_counts_batch(gts, sets, align=16)
    for got, g, m in zip(res, gts, sets):
        _same(got, g, m)


def test_all_background_mask_set_and_full_masks():
    from rsis_amd import cityscapes_eval as E
    rng = np.random.default_rng(9)
    gt = _city(rng, (200, 300), 20)
    empty = np.zeros((70, 200, 300), np.uint8)
    got = E.overlap_counts(gt, empty)
    assert not got[0][:-1].any() and got[0][-1].sum() == 200 * 300
    _same(got, gt, empty)
    full = np.ones((3, 200, 300), np.uint8)
    _same(E.overlap_counts(gt, full), gt, full)
    noise = (rng.random((66, 200, 300)) < 0.5).astype(np.uint8)      # no runs at all
    _same(E.overlap_counts(gt, noise), gt, noise)


def test_job_that_does_not_fit_is_skipped_and_bad_arguments_are_refused():
    from rsis_amd import cityscapes_eval as E
    from rsis_amd._lib import lib, ptr, stream
    L = lib()
    rng = np.random.default_rng(4)
    gts = [_city(rng, (40, 50), 4) for _ in range(3)]
    sets = [_blobs(rng, (40, 50), 3) for _ in range(3)]
    want = [C.np_counts(g, m) for g, m in zip(gts, sets)]
    S = [len(w[1]) for w in want]
    jobs, length, blk, pblk, cnt = E.job_table([2000] * 3, [3] * 3, S)
    pool = torch.zeros((length,), dtype=torch.uint8)
    lut = np.full((3, 65536), 65535, np.uint16)
    for j, g in enumerate(gts):
        pool[jobs[j, 0]:jobs[j, 0] + 4000] = torch.from_numpy(g.reshape(-1).view(np.uint8))
        lut[j, want[j][1]] = np.arange(S[j])
    pool = pool.cuda()
    dlut = torch.from_numpy(lut.view(np.int16)).cuda()
    bits = torch.cat([E._pack_masks(m, (40, 50), "m", torch.device("cuda"))[0] for m in sets])
    counts = torch.full((cnt,), 7, dtype=torch.int32, device="cuda")
    flags = torch.full((3 * 65536,), 7, dtype=torch.uint8, device="cuda")

    def run(J):
        dj = torch.from_numpy(J).cuda()
        assert L.rsis_inst_presence_batch(ptr(pool), pool.numel(), ptr(dj), 3, pblk, ptr(flags), flags.numel(), stream()) == 0
        assert L.rsis_inst_overlap_batch(ptr(pool), pool.numel(), ptr(dj), 3, blk, ptr(dlut), dlut.numel(), ptr(bits), bits.numel(), ptr(counts),
                                         counts.numel(), stream()) == 0
        c, f = counts.cpu().numpy(), flags.view(3, 65536).cpu().numpy()
        return [c[jobs[j, 7]:jobs[j, 7] + 4 * S[j]].reshape(4, S[j]) for j in range(3)], f
    tabs, f = run(jobs)
    for j in range(3):
        assert np.array_equal(tabs[j], want[j][0]) and np.array_equal(np.flatnonzero(f[j]), want[j][1])
    for col, val in ((0, length - 100), (0, 1), (3, bits.numel() - 10), (7, cnt - 5), (2, 3 * 65536 - 100), (4, 1), (6, 0), (6, 65536)):
        bad = jobs.copy()
        bad[1, col] = val                                            # image 1 would leave a buffer (or is misaligned): it touches nothing
        tabs, f = run(bad)
        lo, hi = jobs[1, 7], jobs[1, 7] + 4 * S[1]
        assert not counts[lo:hi].cpu().numpy().any(), (col, val)
        if col in (0, 2):
            assert not f[1].any()
        for j in (0, 2):
            assert np.array_equal(tabs[j], want[j][0]) and np.array_equal(np.flatnonzero(f[j]), want[j][1])
    counts.fill_(7)
    flags.fill_(7)
    dj = torch.from_numpy(jobs).cuda()
    ARG = 1
    assert L.rsis_inst_overlap_blocks(0, 3) == 0 and L.rsis_inst_overlap_blocks(16384, 0) == 1 and L.rsis_inst_overlap_blocks(16385, 65) == 4
    assert L.rsis_inst_presence_batch(None, pool.numel(), ptr(dj), 3, pblk, ptr(flags), flags.numel(), stream()) == ARG
    assert L.rsis_inst_presence_batch(ptr(pool) + 2, pool.numel() - 16, ptr(dj), 3, pblk, ptr(flags), flags.numel(), stream()) == ARG
    assert L.rsis_inst_presence_batch(ptr(pool), pool.numel() - 2, ptr(dj), 3, pblk, ptr(flags), flags.numel(), stream()) == ARG
    assert L.rsis_inst_presence_batch(ptr(pool), pool.numel(), ptr(dj), 3, 0, ptr(flags), flags.numel(), stream()) == ARG
    assert L.rsis_inst_presence_batch(ptr(pool), pool.numel(), ptr(dj), 3, pblk, ptr(flags), 100, stream()) == ARG
    assert L.rsis_inst_overlap_batch(ptr(pool), pool.numel(), None, 3, blk, ptr(dlut), dlut.numel(), ptr(bits), bits.numel(), ptr(counts),
                                     counts.numel(), stream()) == ARG
    assert L.rsis_inst_overlap_batch(ptr(pool), pool.numel(), ptr(dj), 3, blk, None, dlut.numel(), ptr(bits), bits.numel(), ptr(counts),
                                     counts.numel(), stream()) == ARG
    assert L.rsis_inst_overlap_batch(ptr(pool), pool.numel(), ptr(dj), 3, blk, ptr(dlut), dlut.numel(), None, bits.numel(), ptr(counts),
                                     counts.numel(), stream()) == ARG
    assert L.rsis_inst_overlap_batch(ptr(pool), pool.numel(), ptr(dj), 0, blk, ptr(dlut), dlut.numel(), ptr(bits), bits.numel(), ptr(counts),
                                     counts.numel(), stream()) == ARG
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and bool((flags == 7).all())
    with pytest.raises(ValueError):
        E.overlap_counts(gts[0], np.zeros((2, 8, 8), np.uint8))       # masks of another size
    with pytest.raises(ValueError):
        E.overlap_counts(np.zeros((4, 4), np.float32), np.zeros((0, 4, 4), np.uint8))


def test_evaluate_dirs_and_cli_on_a_folder_written_from_the_fixture(tmp_path):
    from rsis_amd import cityscapes_eval as E
    case = C.load_cases()[0]
    res, gt_dir = C.write_folder(str(tmp_path), case["images"])
    out = E.evaluate_dirs(res, gt_dir)
    assert np.array_equal(np.isnan(out["aps"]), np.isnan(case["aps"])) and np.nanmax(np.abs(out["aps"] - case["aps"])) <= 1e-12
    assert abs(out["averages"]["allAp"] - case["all"][0]) <= 1e-12
    name = str(tmp_path / "cli.json")
    p = subprocess.run([sys.executable, "-m", "rsis_amd.cityscapes_eval", "--results", res, "--gt", gt_dir, "--json", name], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert E.summary(out["averages"]) in p.stdout
    E.write_result_json(str(tmp_path / "here.json"), out)
    assert json.load(open(name)) == json.load(open(str(tmp_path / "here.json")))


def test_synthetic_driver_scores_what_it_wrote(tmp_path):
    """rsis_amd.eval_cityscapes with --synthetic on a tiny model: create_figures keeps its return value, writes the 16-bit ground truth,
    score() prints the table and writes the JSON; scoring the folder with the CLI gives the same JSON; the golden module agrees;
    --no_run_coco_eval scores nothing."""
    from PIL import Image
    from rsis_amd.args import get_parser
    from rsis_amd import cityscapes_eval as E, eval_cityscapes
    models = str(tmp_path / "models")
    argv = ["--synthetic", "-model_name", "cs", "-batch_size", "2", "-maxseqlen", "3", "-hidden_size", "32", "-synthetic_batches", "8",
            "-num_classes", "9", "-imsize", "64", "-models_root", models]
    a = get_parser().parse_args(argv)
    torch.manual_seed(a.seed)
    ev = eval_cityscapes.Evaluate(a)
    assert ev.create_figures() == 4 * 3 * 8                          # images x timesteps x foreground classes
    res = ev.score()
    assert res["images"] == 4 and res["aps"].shape == (8, 10)
    mine = os.path.join(models, "cs", "cs_cityscapes_eval.json")
    assert os.path.exists(mine)
    gt_dir, results = os.path.join(models, "cs", "cs_gt"), os.path.join(models, "cs", "cs_results")
    with Image.open(os.path.join(gt_dir, "synthetic_000000_gtFine_instanceIds.png")) as im:
        assert im.mode.startswith("I;16") and im.size == (128, 128)
        g = np.array(im)
    assert g.dtype == np.uint16 and C.ROAD in g and g.max() >= 24000 and np.array_equal(g[::2, ::2], g[1::2, 1::2])
    cli = str(tmp_path / "cli.json")
    p = subprocess.run([sys.executable, "-m", "rsis_amd.cityscapes_eval", "--results", results, "--gt", gt_dir, "--json", cli], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert json.load(open(cli)) == json.load(open(mine))
    # the golden module on the files
    images = []
    for stem, txt, gtf in E.pair_files(results, gt_dir):
        preds = [(np.array(Image.open(png)), lab, sc) for png, lab, sc in E.parse_result_txt(txt)]
        images.append((np.array(Image.open(gtf)), preds))
    want = G.evaluate(images)["aps"]
    assert np.array_equal(np.isnan(want), np.isnan(res["aps"]))
    assert np.all(np.abs(want[~np.isnan(want)] - res["aps"][~np.isnan(want)]) <= 1e-12)
    b = get_parser().parse_args(argv + ["--no_run_coco_eval", "-model_name", "cs2"])
    ev2 = eval_cityscapes.Evaluate(b)
    assert ev2.create_figures() == 4 * 3 * 8 and ev2.records == [] and ev2.score() is None
    assert not os.path.exists(os.path.join(models, "cs2", "cs2_cityscapes_eval.json"))
