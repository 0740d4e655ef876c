"""COCO segm evaluation on the device (rsis_amd/csrc/maskeval.hip, rsis_amd/cocoeval.py, wired into rsis_amd.eval) against the
reference's own COCOeval (tests/golden/cocoeval.npz, tools/make_golden_cocoeval.py): integer intersections and one IEEE division,
so IoUs are compared bit for bit and matches / flags for equality; stats within 1e-11 (means of at most 10 * 101 * 20 values in
[0, 1]: the worst-case summation-order error is n * 2^-53, about 2e-12)."""
import io
import json
import os

import numpy as np
import pytest
import torch

from cocoeval_golden import load
from rsis_amd import cocoeval as CE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _unpack(words, length):
    """(n, words) int64 bit words -> (n, length) uint8, on the host"""
    w = words.cpu().numpy().view(np.uint64)
    b = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")
    assert not b[:, length:].any(), "tail bits must be zero"
    return b[:, :length]


def test_pack_bits_and_rle_to_bits_agree_with_numpy():
    z = np.load(os.path.join(GOLDEN, "rle.npz"))
    for k in range(int(z["n"])):
        m = z["mask%d" % k]
        col = np.ascontiguousarray(m.T).reshape(1, -1)              # column-major element order, as rsis_mask_resize_threshold writes
        n = col.shape[1]
        stack = np.concatenate([col, 1 - col, np.zeros_like(col), np.ones_like(col) * 255], axis=0).astype(np.uint8)
        words, area = CE.pack_bits(torch.from_numpy(stack).cuda())
        assert words.shape == (4, CE.words_of(n))
        assert np.array_equal(_unpack(words, n), (stack != 0).astype(np.uint8)), k
        assert area.cpu().tolist() == [int(col.sum()), n - int(col.sum()), 0, n], k
        rows, rarea = CE.rle_to_bits([z["counts%d" % k], CE.rle_from_string(bytes(z["string%d" % k]))], [n, n])
        assert torch.equal(rows[0], words[0]) and torch.equal(rows[1], words[0]), k
        assert rarea.cpu().tolist() == [int(col.sum())] * 2
    # rows that do not start on a 16-byte boundary (odd length) and several masks of different sizes in one launch
    r = np.random.default_rng(5)
    masks = [(r.uniform(size=(n,)) < 0.4).astype(np.uint8) for n in (1, 63, 64, 65, 127, 1961, 37 * 53, 70001)]
    from oracle import rle_numpy
    counts = [rle_numpy.rle_counts(m.reshape(-1, 1)) for m in masks]
    rows, area = CE.rle_to_bits(counts, [len(m) for m in masks])
    for m, row, a in zip(masks, rows, area.cpu().tolist()):
        assert np.array_equal(_unpack(row.reshape(1, -1), len(m))[0], m) and a == int(m.sum())
    odd = (r.uniform(size=(5, 1961)) < 0.5).astype(np.uint8)
    words, area = CE.pack_bits(torch.from_numpy(odd).cuda())
    assert np.array_equal(_unpack(words, 1961), odd) and area.cpu().tolist() == odd.sum(axis=1).tolist()


def _evaluator(S, run, gt=None, dt=None):
    ev = CE.COCOEvalDevice(S["gt"] if gt is None else gt, S["dt"] if dt is None else dt)
    ev.params.maxDets = list(run["maxDets"])
    ev.params.useCats = run["useCats"]
    ev.params.imgIds = list(run["imgIds"])
    ev.params.catIds = list(run["catIds"])
    return ev


def _check_cells(ev, run):
    cats = run["catIds"] if run["useCats"] else [-1]
    n = 0
    for img in run["imgIds"]:
        for c in cats:
            want, got = run["ious"][n], ev.iou_matrix(img, c)
            n += 1
            if want.size == 0:
                assert np.asarray(got).size == 0
                continue
            got = np.asarray(got)
            assert got.dtype == np.float64 and got.shape == want.shape
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (img, c)       # bit-equal
    cells = ev.evalImgs
    assert len(cells) == len(run["cells"])
    for e, w in zip(cells, run["cells"]):
        assert (e is None) == (w is None)
        if w is None:
            continue
        assert e["dtIds"] == w["dtIds"].tolist() and e["gtIds"] == w["gtIds"].tolist()
        assert np.array_equal(e["dtMatches"], w["dtMatches"]) and np.array_equal(e["gtMatches"], w["gtMatches"])
        assert np.array_equal(e["dtIgnore"].astype(np.int64), w["dtIgnore"]) and np.array_equal(e["gtIgnore"], w["gtIgnore"])
        assert np.array_equal(np.asarray(e["dtScores"]), w["dtScores"])


def test_ious_matches_and_stats_equal_the_reference():
    sets, runs = load()
    for run in runs:
        ev = _evaluator(sets[run["set"]], run)
        ev.evaluate()
        _check_cells(ev, run)
        ev.accumulate()
        assert np.array_equal(ev.eval["precision"], run["precision"])
        assert np.array_equal(ev.eval["recall"], run["recall"])
        text = io.StringIO()
        stats = ev.summarize(text)
        for s, w in zip(stats, run["stats"]):
            print("stat %.17g reference %.17g" % (s, w))
        assert np.abs(stats - run["stats"]).max() <= 1e-11
        assert text.getvalue().splitlines() == run["summary"]


def _decode(rec):
    c = CE.rle_from_string(rec["segmentation"]["counts"])
    v = np.zeros((int(c.sum()),), np.uint8)
    pos = np.concatenate([np.zeros((1,), np.int64), np.cumsum(c.astype(np.int64))])
    for j in range(1, len(c), 2):
        v[pos[j]:pos[j + 1]] = 1
    return v


def test_device_tensor_path_equals_json_path():
    sets, runs = load()
    for run in runs[1:4]:
        S = sets[run["set"]]
        ev = CE.COCOEvalDevice()
        for img in run["imgIds"]:
            g = [r for r in S["gt"] if r["image_id"] == img]
            d = [r for r in S["dt"] if r["image_id"] == img]
            if g:
                ev.add_gt_masks(img, torch.from_numpy(np.stack([_decode(r) for r in g])).cuda(), [r["category_id"] for r in g],
                                area=[r["area"] for r in g], iscrowd=[r["iscrowd"] for r in g], ignore=[r.get("ignore", 0) for r in g],
                                ids=[r["id"] for r in g])
            if d:                                                   # records that share a mask share its row, as in rsis_amd.eval
                uniq, rows = {}, []
                for r in d:
                    rows.append(uniq.setdefault(r["segmentation"]["counts"], len(uniq)))
                first = {}
                for k, v in enumerate(rows):
                    first.setdefault(v, k)
                m = np.stack([_decode(d[first[j]]) for j in range(len(uniq))])
                ev.add_dt_masks(img, torch.from_numpy(m).cuda(), [r["category_id"] for r in d], [r["score"] for r in d], rows=rows)
        # detection ids count records in the order given: the JSON set lists them image by image too
        ev.params.maxDets, ev.params.useCats = list(run["maxDets"]), run["useCats"]
        ev.params.imgIds, ev.params.catIds = list(run["imgIds"]), list(run["catIds"])
        ev.evaluate()
        _check_cells(ev, run)
        ev.accumulate()
        assert np.array_equal(ev.eval["precision"], run["precision"]) and np.array_equal(ev.eval["recall"], run["recall"])


def test_known_answers():
    """detections equal to the ground truth with score 1: AP = AR = 1; shifted off every ground truth: 0"""
    sets, runs = load()
    S = sets[1]
    gt = S["gt"]
    same = [dict(image_id=r["image_id"], category_id=r["category_id"], segmentation=r["segmentation"], score=1.0) for r in gt]
    ev = CE.COCOEvalDevice(gt, same)
    ev.evaluate().accumulate().summarize(io.StringIO())
    # (precision is tp / (tp + fp + eps): one ulp below 1 where tp = 1; the bound is the one stated for stats above)
    assert all(abs(ev.stats[j] - 1.0) <= 1e-11 for j in (0, 1, 3, 5, 6, 9)) and ev.stats[7] == 1.0 and ev.stats[10] == 1.0
    off = []
    for r in gt:
        h, w = r["segmentation"]["size"]
        m = _decode(r).reshape(w, h)
        free = 1 - np.clip(sum(_decode(q).reshape(w, h) for q in gt if q["image_id"] == r["image_id"]), 0, 1)
        assert free.sum() > 0 and m.sum() > 0
        text = CE.rle_to_string(_counts(free.reshape(-1).astype(np.uint8))).decode("ascii")
        off.append(dict(image_id=r["image_id"], category_id=r["category_id"], segmentation={"size": [h, w], "counts": text}, score=1.0))
    ev = CE.COCOEvalDevice(gt, off)
    ev.evaluate().accumulate().summarize(io.StringIO())
    assert ev.stats[0] == 0.0 and ev.stats[1] == 0.0 and ev.stats[7] == 0.0


def _counts(v):
    from oracle import rle_numpy
    return rle_numpy.rle_counts(v.reshape(-1, 1))


def _args(tmp_path, *extra):
    from rsis_amd.args import get_parser
    a = get_parser().parse_args(["--synthetic", "-model_name", "cocotest", "-batch_size", "2", "-maxseqlen", "3", "-hidden_size", "32",
                                 "-synthetic_batches", "8", "-synthetic_instances", "3", "-stop_th", "0.0", "-class_th", "0.0",
                                 "-min_size", "0.0"] + list(extra))
    a.models_root, a.imsize, a.num_classes = str(tmp_path), 64, 5
    return a


def _stand_in_network(ev, mode):
    """replaces inference (rsis_amd.eval_common.test) by masks made from the loader's targets, so that the evaluation has a known answer:
    'exact' = the ground truth with score 1 for its class, 'off' = the region no ground truth covers, 'noisy' = the ground truth
    shifted by a few pixels with spread-out class scores"""
    table = {b[0].data_ptr(): b for b in ev.loader.batches}

    def fake(args, _enc, _dec, x):
        _x, y_mask, y_class, _sw, _ = table[x.data_ptr()]
        B, T, C = x.shape[0], args.maxseqlen, args.num_classes
        m = y_mask[:, :T].reshape(B, T, 64, 64).clone()
        onehot = torch.nn.functional.one_hot(y_class[:, :T], C).to(torch.float32)
        scores = onehot
        if mode == "off":
            m = (1 - m.sum(dim=1, keepdim=True).clamp(max=1)).expand(B, T, 64, 64).contiguous()
        elif mode == "noisy":
            for t in range(T):
                m[:, t] = torch.roll(m[:, t], shifts=2 * t + 1, dims=-1)
            g = torch.Generator().manual_seed(3)
            scores = torch.rand((B, T, C), generator=g).to(x.device) + 0.7 * onehot
            scores = scores / scores.sum(dim=-1, keepdim=True)
        return m, scores, torch.ones((B, T, 1), device=x.device)
    return fake


def _run(tmp_path, *extra, mode=None, monkeypatch=None):
    from rsis_amd.eval import Evaluate
    torch.manual_seed(0)
    ev = Evaluate(_args(tmp_path, *extra))
    if mode is not None:
        monkeypatch.setattr("rsis_amd.eval_common.test", _stand_in_network(ev, mode))
    preds = ev.run_eval()
    path = os.path.join(str(tmp_path), "cocotest", "cocotest_test_cocoeval.json")
    return ev, preds, (json.load(open(path)) if os.path.exists(path) else None)


def _gt_records(ev):
    """the loader's targets as COCO records (host restatement of what run_eval feeds the evaluator)"""
    out, acc = [], 0
    for _x, y_mask, y_class, sw_mask, _sw in ev.loader:
        for s in range(y_mask.shape[0]):
            for g in range(int((sw_mask[s] > 0).sum())):
                m = (y_mask[s, g].reshape(64, 64) > 0.5).cpu().numpy().astype(np.uint8)
                out.append(dict(image_id=ev.sample_list[acc + s], category_id=int(y_class[s, g]), id=len(out) + 1,
                                segmentation={"size": [64, 64], "counts": CE.rle_to_string(_counts(m.T.reshape(-1))).decode("ascii")}))
        acc += y_mask.shape[0]
    return out


def test_eval_driver_runs_the_evaluation(tmp_path):
    """the real network (random weights): the file is written, 13 stats, the reference's parameters"""
    ev, preds, res = _run(tmp_path / "a")
    assert res is not None and len(res["stats"]) == 13 and len(preds) == 4 * 3 * 4
    assert all(np.isfinite(v) and (v == -1 or 0 <= v <= 1) for v in res["stats"])
    assert res["params"]["maxDets"] == [1, 100, 100] and res["params"]["useCats"] == 1 and res["per_class"] == {}
    _, _, res3 = _run(tmp_path / "c", "--all_classes")
    assert sorted(res3["per_class"]) == ["1", "2", "3", "4"] and all(len(v) == 13 for v in res3["per_class"].values())


def test_eval_driver_flags_and_fast_path(tmp_path, monkeypatch):
    """--ignore_cats and -max_dets change the stats the way the evaluation of the WRITTEN predictions file says: the fast path (device
    masks, one row per predicted mask) and the JSON path agree"""
    seen = {}
    for name, extra, use_cats, max_dets in (("cats", (), 1, 100), ("nocats", ("--ignore_cats",), 0, 100),
                                            ("nocats2", ("-max_dets", "2", "--ignore_cats"), 0, 2)):
        ev, preds, res = _run(tmp_path / name, *extra, mode="noisy", monkeypatch=monkeypatch)
        with open(os.path.join(str(tmp_path / name), "cocotest", "cocotest_test_predictions.json")) as f:
            written = json.load(f)
        ref = CE.COCOEvalDevice(_gt_records(ev), written)
        ref.params.maxDets, ref.params.useCats = [1, max_dets, 100], use_cats
        ref.params.imgIds, ref.params.catIds = sorted(ev.sample_list), list(range(1, 5))
        ref.evaluate().accumulate().summarize(io.StringIO())
        print(name, res["stats"])
        assert np.array_equal(np.asarray(res["stats"]), ref.stats)
        assert res["params"]["maxDets"] == sorted([1, max_dets, 100]) and res["params"]["useCats"] == use_cats
        seen[name] = np.asarray(res["stats"])
    assert 0 < seen["cats"][0] < 1 and 0 < seen["nocats"][0] < 1
    assert not np.array_equal(seen["cats"], seen["nocats"])
    assert seen["nocats2"][7] < seen["nocats"][7]                   # 2 detections cannot recall 3 ground truths per image


def test_eval_driver_known_answers(tmp_path, monkeypatch):
    _, _, res = _run(tmp_path / "exact", mode="exact", monkeypatch=monkeypatch)
    print("exact", res["stats"])
    assert all(abs(res["stats"][j] - 1.0) <= 1e-11 for j in (0, 1, 3, 5, 6, 9)) and res["stats"][7] == 1.0 and res["stats"][10] == 1.0
    _, _, res = _run(tmp_path / "off", mode="off", monkeypatch=monkeypatch)
    print("off", res["stats"])
    assert res["stats"][0] == 0.0 and res["stats"][1] == 0.0 and res["stats"][7] == 0.0


def test_no_run_coco_eval(tmp_path):
    ev, preds, res = _run(tmp_path, "--no_run_coco_eval")
    assert res is None and ev.coco is None and len(preds) > 0
    assert os.path.exists(os.path.join(str(tmp_path), "cocotest", "cocotest_test_predictions.json"))
