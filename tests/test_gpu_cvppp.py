"""CVPPP measures on the device (rsis_amd/csrc/labeleval.hip through rsis_amd/cvppp_eval.py) against the float64 numpy statement of
their definitions (tests/cvppp_golden.py).  Every count is an integer and every score one fixed-order float64 expression of integers,
so everything here is compared for EQUALITY: counts array_equal, scores == with NaN in the same places.  No tolerance anywhere."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import cvppp_golden as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _leafy(rng, h, w, k, background=0.8):
    """k rectangular 'leaves' (labels 1 .. k) covering about 1 - background of the image"""
    lab = np.zeros((h, w), np.uint8)
    side = max(1, int(np.sqrt((1.0 - background) * h * w / max(k, 1)) * 1.15))
    for n in range(1, k + 1):
        y, x = int(rng.integers(0, max(1, h - side))), int(rng.integers(0, max(1, w - side)))
        lab[y:y + side, x:x + side] = n
    return lab


def _perturbed(rng, g):
    r = np.roll(g, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1)).copy()
    k = int(g.max())
    if k >= 2:
        r[r == k] = k - 1                                          # two leaves merged: a gap-free but shorter range
    return r


def _check(ins, gts, align=16):
    from rsis_amd import cvppp_eval as E
    t = E.contingency(ins, gts, align=align)
    s = E.score_pairs(ins, gts, align=align)
    assert t.dtype == torch.int64 and tuple(t.shape) == (len(gts), 256, 256) and tuple(s.shape) == (len(gts), 6) and s.dtype == torch.float64
    for p, (a, g) in enumerate(zip(ins, gts)):
        a, g = np.asarray(torch.as_tensor(a).cpu()), np.asarray(torch.as_tensor(g).cpu())
        want_t = G.counts(a if a.shape == g.shape else G.nearest_resize(a, *g.shape), g)
        assert np.array_equal(t[p].cpu().numpy(), want_t), "counts of pair %d (%s)" % (p, g.shape)
        want = G.scores_from_counts(want_t)
        got = s[p].numpy()
        print("pair %d %s: device %s numpy %s" % (p, g.shape, got.tolist(), want.tolist()))
        assert G.same_scores(got, want), "scores of pair %d: %s != %s" % (p, got.tolist(), want.tolist())
    return t, s


def test_fixture_counts_and_scores_are_equal():
    from rsis_amd import cvppp_eval as E
    cases = G.load()
    ins, gts = [torch.from_numpy(c["in"]) for c in cases], [torch.from_numpy(c["gt"]) for c in cases]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        t = E.contingency(ins, gts)
        s = E.score_pairs(ins, gts)
    assert sum("nearest rule" in str(x.message) for x in w) == 2          # the one pair of unequal sizes, once per call
    for p, c in enumerate(cases):
        assert np.array_equal(t[p].cpu().numpy(), c["counts"]), c["name"]
        assert G.same_scores(s[p].numpy(), c["scores"]), (c["name"], s[p].tolist(), c["scores"].tolist())
    # device tensors go the same way
    s2 = E.score_pairs([x.cuda() for x in ins], [x.cuda() for x in gts])
    assert G.same_scores(s2.numpy(), s.numpy())


def test_sizes_that_are_not_multiples_of_16():
    rng = np.random.default_rng(1)
    ins, gts = [], []
    for h, w in ((1, 1), (1, 15), (1, 17), (3, 5), (1, 1961), (37, 53), (500, 530), (16, 16), (1, 31), (1, 33)):
        g = _leafy(rng, h, w, int(rng.integers(1, 9)))
        gts.append(torch.from_numpy(g))
        ins.append(torch.from_numpy(_perturbed(rng, g)))
    _check(ins, gts)


def test_many_pairs_of_different_sizes_in_one_launch_unaligned():
    """align = 1 packs the pool back to back: image starts at every offset modulo 16, `in` and `gt` of a pair at DIFFERENT offsets
    modulo 16 (the path that cuts gt's 16 bytes out of two aligned cells), the last cell at the very end of the pool"""
    rng = np.random.default_rng(2)
    ins, gts = [], []
    for p in range(48):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 90))
        if p == 47:
            h, w = 29, 33                                          # odd pixel count last: its gt ends the pool
        g = _leafy(rng, h, w, int(rng.integers(1, 20)), background=0.6)
        gts.append(torch.from_numpy(g))
        ins.append(torch.from_numpy(_perturbed(rng, g)))
    from rsis_amd import cvppp_eval as E
    jobs, _length, _blocks = E.job_table([g.numel() for g in gts], align=1)
    assert len(set(int(v) % 16 for v in jobs[:, 0])) >= 8 and any((int(a) - int(b)) % 16 for a, b in zip(jobs[:, 0], jobs[:, 1]))
    _, s1 = _check(ins, gts, align=1)
    _, s16 = _check(ins, gts, align=16)
    assert G.same_scores(s1.numpy(), s16.numpy())


def test_labels_over_the_whole_range():
    """labels outside the 64 x 64 LDS window take the direct path; mixed with in-window labels in one image"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (123, 211)).astype(np.uint8)
    g = rng.integers(0, 256, (123, 211)).astype(np.uint8)
    b = _leafy(rng, 200, 210, 12)
    b2 = _perturbed(rng, b)
    b2[b2 == 3] = 200                                              # a few labels far outside the window, in runs
    hi = (_leafy(rng, 64, 100, 5) * 50).astype(np.uint8)           # {0, 50, 100, 150, 200, 250}
    _check([torch.from_numpy(x) for x in (a, b2, hi, np.full((9, 9), 255, np.uint8))],
           [torch.from_numpy(x) for x in (g, b, np.roll(hi, 2, 1).copy(), np.full((9, 9), 255, np.uint8))])


def test_a3_sized_pair_mostly_background_and_same_bits_twice():
    """2448 x 2048, 80 % background: many blocks per pair, all of them adding to the (0, 0) cell; and the launch repeated"""
    from rsis_amd import cvppp_eval as E
    rng = np.random.default_rng(4)
    g = _leafy(rng, 2048, 2448, 30, background=0.8)
    r = _perturbed(rng, g)
    assert 0.7 < float((g == 0).mean()) < 0.9
    ins, gts = [torch.from_numpy(r), torch.from_numpy(r[:700, :900].copy())], [torch.from_numpy(g), torch.from_numpy(g[:700, :900].copy())]
    assert E.job_table([g.size])[2] >= 64                          # blocks of the large pair
    t1, s1 = _check(ins, gts)
    t2, s2 = E.contingency(ins, gts), E.score_pairs(ins, gts)
    assert torch.equal(t1, t2) and np.array_equal(s1.numpy().view(np.int64), s2.numpy().view(np.int64))


def test_out_of_range_job_is_skipped_and_bad_arguments_are_refused():
    from rsis_amd import cvppp_eval as E
    from rsis_amd._lib import lib, ptr, stream
    L = lib()
    rng = np.random.default_rng(5)
    gts = [torch.from_numpy(_leafy(rng, 40, 50, 4)) for _ in range(3)]
    ins = [torch.from_numpy(_perturbed(rng, g.numpy())) for g in gts]
    pool, jobs, n, blocks = E._pool(ins, gts, 16, torch.device("cuda"))
    bad = jobs.clone()
    bad[1, 1] = pool.numel() - 100                                 # gt of pair 1 would end past the pool: skipped, nothing of it is read
    counts = torch.full((n * E.TABLE,), 7, dtype=torch.int32, device="cuda")
    scores = torch.full((n, 6), 7.0, dtype=torch.float64, device="cuda")
    assert L.rsis_label_contingency_batch(ptr(pool), pool.numel(), ptr(bad), n, blocks, ptr(counts), counts.numel(), stream()) == 0
    assert L.rsis_label_scores_batch(ptr(counts), counts.numel(), ptr(bad), n, ptr(scores), stream()) == 0
    t = counts.view(n, 256, 256).cpu().numpy()
    assert not t[1].any() and not scores[1].cpu().numpy().any()    # zeroed by the call, left alone by the skipped job
    for p in (0, 2):
        want = G.counts(ins[p].numpy(), gts[p].numpy())
        assert np.array_equal(t[p], want) and G.same_scores(scores[p].cpu().numpy(), G.scores_from_counts(want))
    bad2 = jobs.clone()
    bad2[2, 3] = n * E.TABLE - 100                                 # a table that would end past counts: skipped by both launches
    assert L.rsis_label_contingency_batch(ptr(pool), pool.numel(), ptr(bad2), n, blocks, ptr(counts), counts.numel(), stream()) == 0
    assert L.rsis_label_scores_batch(ptr(counts), counts.numel(), ptr(bad2), n, ptr(scores), stream()) == 0
    assert not scores[2].cpu().numpy().any() and np.array_equal(counts.view(n, 256, 256)[0].cpu().numpy(), G.counts(ins[0].numpy(), gts[0].numpy()))
    # refused before anything is launched: the outputs keep their marker
    counts.fill_(7)
    scores.fill_(7.0)
    ARG = 1
    assert L.rsis_label_contingency_batch(None, pool.numel(), ptr(jobs), n, blocks, ptr(counts), counts.numel(), stream()) == ARG
    assert L.rsis_label_contingency_batch(ptr(pool) + 1, pool.numel() - 1, ptr(jobs), n, blocks, ptr(counts), counts.numel(), stream()) == ARG
    assert L.rsis_label_contingency_batch(ptr(pool), pool.numel(), None, n, blocks, ptr(counts), counts.numel(), stream()) == ARG
    assert L.rsis_label_contingency_batch(ptr(pool), pool.numel(), ptr(jobs), 0, blocks, ptr(counts), counts.numel(), stream()) == ARG
    assert L.rsis_label_contingency_batch(ptr(pool), pool.numel(), ptr(jobs), n, 0, ptr(counts), counts.numel(), stream()) == ARG
    assert L.rsis_label_contingency_batch(ptr(pool), pool.numel(), ptr(jobs), n, blocks, None, counts.numel(), stream()) == ARG
    assert L.rsis_label_contingency_batch(ptr(pool), pool.numel(), ptr(jobs), n, blocks, ptr(counts), 100, stream()) == ARG
    assert L.rsis_label_scores_batch(None, counts.numel(), ptr(jobs), n, ptr(scores), stream()) == ARG
    assert L.rsis_label_scores_batch(ptr(counts), counts.numel(), ptr(jobs), n, None, stream()) == ARG
    assert L.rsis_label_scores_batch(ptr(counts), counts.numel(), ptr(jobs), 0, ptr(scores), stream()) == ARG
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and bool((scores == 7.0).all())
    with pytest.raises(ValueError):
        E.score_pairs([torch.zeros((2, 2))], [torch.zeros((2, 2), dtype=torch.uint8)])
    with pytest.raises(ValueError):
        E.score_pairs([], [torch.zeros((2, 2), dtype=torch.uint8)])


def _tree(tmp_path, n=7):
    """a synthesised CVPPP folder and a results folder of perturbed copies: one result missing, one of another size"""
    from PIL import Image
    from rsis_amd.dataloader.leaves import synthesize_leaves_dir
    gt = synthesize_leaves_dir(str(tmp_path / "gt"), n=n, size=(88, 104), seed=11)
    res = tmp_path / "res" / "A1"
    res.mkdir(parents=True)
    rng = np.random.default_rng(6)
    ins, gts = [], []
    for k in range(n):
        g = np.array(Image.open(os.path.join(gt, "plant%03d_label.png" % k)))
        r = _perturbed(rng, g)
        if k == 2:
            r = np.zeros_like(g)                                   # no file: scored against zeros
        else:
            if k == 4:
                r = r[::2, ::2].copy()                             # another size: the nearest rule
            Image.fromarray(r).save(str(res / ("plant%03d_label.png" % k)))
        ins.append(r)
        gts.append(g)
    return gt, str(tmp_path / "res"), ins, gts


def test_evaluate_dirs_and_cli(tmp_path):
    from rsis_amd import cvppp_eval as E
    gt, res, ins, gts = _tree(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        numbers, scores = E.evaluate_dirs(res, gt)
    want = G.score_pairs(ins, gts)
    assert numbers == list(range(7)) and G.same_scores(scores.numpy(), want)
    out = tmp_path / "csv"
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "rsis_amd.cvppp_eval", "--results", res, "--gt", gt, "--user", "tester", "--out", str(out)],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert p.returncode == 0, p.stderr
    text = open(str(out / "tester_A1_results.csv")).read()
    assert text == E.result_table_text(list(range(7)), want)
    lines = [l for l in p.stdout.splitlines() if l.split(",")[0] in E.SUMMARY_ROWS]
    assert lines == text.splitlines()[-5:] and "no result image" in p.stdout


def test_evaluate_score_after_create_figures(tmp_path):
    """rsis_amd.eval_leaves.Evaluate end to end (the checkpoint set-up of tests/test_maskpost.py): create_figures() keeps its return
    value, score() scores those files against the split's ground truth, prints and writes <model_name>_A1_results.csv"""
    from PIL import Image
    from rsis_amd.args import get_parser
    from rsis_amd.dataloader.leaves import synthesize_leaves_dir
    from rsis_amd.modules import FeatureExtractor, RSIS
    from rsis_amd.utils.utils import save_checkpoint
    from rsis_amd import cvppp_eval as E, eval_leaves
    d = synthesize_leaves_dir(str(tmp_path / "A1"), n=101, size=(80, 96), seed=5)
    models = str(tmp_path / "models")
    a = get_parser().parse_args(["-model_name", "lv", "-dataset", "leaves", "-leaves_dir", d, "-leaves_test_dir", d, "-eval_split", "val",
                                 "-batch_size", "2", "-maxseqlen", "4", "-gt_maxseqlen", "6", "-num_classes", "2", "-imsize", "64",
                                 "--resize", "-hidden_size", "32", "-num_workers", "2", "-class_th", "0.0", "-models_root", models])
    torch.manual_seed(3)
    enc, dec = FeatureExtractor(a).cuda(), RSIS(a).cuda()
    a.epoch_resume, a.best_val_loss = 0, 0.0
    save_checkpoint(a, enc, dec, torch.optim.Adam(enc.parameters()), torch.optim.Adam(dec.parameters()), root=models)
    ev = eval_leaves.Evaluate(a)
    written = ev.create_figures()
    assert len(written) == 5 and all(p.endswith("_label.png") for p in written)
    numbers, scores = ev.score(written)
    assert numbers == [96, 97, 98, 99, 100] and tuple(scores.shape) == (5, 6)
    ins = [np.array(Image.open(p)) for p in written]
    gts = [np.array(Image.open(p)) for p in ev.dataset.gt_files]
    want = G.score_pairs(ins, gts)
    assert G.same_scores(scores.numpy(), want)
    csv = os.path.join(models, "lv", "lv_results", "lv_A1_results.csv")
    assert open(csv).read() == E.result_table_text(numbers, want)
    # a split without ground truth has nothing to score
    ev.dataset.gt_files, ev.split = [], "test"
    assert ev.score(written) is None


def test_evaluate_doubles_a_lone_tail_image(tmp_path, monkeypatch):
    """eval_leaves over a val split of 3 images at batch 2 with a stand-in for test() that records what it is given: the lone last image
    arrives twice, the copy's outputs are dropped -- one label image per sample, each from its own masks (image k's mask covers the top
    8 * (k + 1) of 32 rows)"""
    from PIL import Image
    from rsis_amd.args import get_parser
    from rsis_amd.dataloader.leaves import synthesize_leaves_dir
    from rsis_amd import eval_leaves
    d = synthesize_leaves_dir(str(tmp_path / "A1"), n=99, size=(40, 48), seed=5)
    a = get_parser().parse_args(["-model_name", "lv", "-dataset", "leaves", "-leaves_dir", d, "-leaves_test_dir", d, "-eval_split", "val",
                                 "-batch_size", "2", "-maxseqlen", "3", "-gt_maxseqlen", "6", "-num_classes", "2", "-imsize", "32",
                                 "--resize", "-hidden_size", "32", "-num_workers", "2", "-class_th", "0.0",
                                 "-models_root", str(tmp_path / "models")])
    torch.manual_seed(3)
    ev = eval_leaves.Evaluate(a)
    assert len(ev.sample_list) == 3 and len(ev.loader) == 2
    seen, twins = [], []

    def fake(args, encoder, decoder, x, return_logits=False):
        k0, B, T = sum(s[0] for s in seen), x.shape[0], args.maxseqlen
        seen.append(tuple(x.shape))
        twins.append(bool((x[0] == x[1]).all()))
        out = torch.zeros((B, T, 32, 32))
        for s in range(B):
            out[s, :, :8 * (k0 + s + 1)] = 1.0
        return out.cuda(), torch.full((B, T, 2), 0.5).cuda(), torch.ones((B, T, 1)).cuda()

    monkeypatch.setattr("rsis_amd.eval_common.test", fake)
    written = ev.create_figures()
    assert seen == [(2, 3, 32, 32), (2, 3, 32, 32)] and twins == [False, True]
    assert len(written) == len(ev.sample_list) == 3
    assert [os.path.basename(p) for p in written] == ["plant%03d_label.png" % i for i in (96, 97, 98)]
    labels = [np.array(Image.open(p)) for p in written]
    assert all(l.shape == (40, 48) for l in labels)
    rows = [int((l > 0).any(axis=1).sum()) for l in labels]
    assert all(abs(r - 10 * (k + 1)) <= 1 for k, r in enumerate(rows)), rows
