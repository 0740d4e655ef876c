"""The --display figures on the device: rsis_overlay_masks / rsis_overlay_moments (csrc/overlay.hip) against their float64 numpy statement
(tests/overlay_golden.py), `encode_masks(want_masks=True)`, `display.save_figure` and `python -m rsis_amd.eval --display` end to end.

Exactness is derived, not measured: with alpha = 2^-b a pixel under m painted masks holds an 8-bit value with b * m fractional bits, so
the fp32 fmaf chain -- and `v + 0.5f` -- is exact while 8 + b * m <= 24 (alpha 0.5: m <= 16; alpha 0.25: m <= 8).  There the device must
EQUAL the numpy statement; under more masks each of the at most k fp32 roundings moves v by <= 2^-17 (half an ulp below 256), which can
only flip the final rounding at a tie: |diff| <= 1 grey level.  The moments are integers and always equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import overlay_golden as G
from rsis_amd import display
from rsis_amd._lib import RsisHipError, check, lib, ptr, stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the smallest shapes at which tiling, layout or width can go wrong (one pixel, one row, one column, odd sizes, a multiple of 64) and
# the ones at which the kernel takes another path: its tile is 128 rows x 32 columns,
# mask loads are 16 bytes wide for h % 16 == 0, 4 bytes for h % 4 == 0, single bytes otherwise
SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 128), (131, 33), (132, 40), (144, 70)]
ORDER = [6, 2, 4, 0, 1]                                         # a non-identity permutation with gaps, from n = 7 masks


def _case(h, w, n, seed, density=0.45, one=1):
    r = np.random.default_rng(seed)
    image = r.integers(0, 256, (h, w, 3), dtype=np.uint8)
    masks = (r.random((n, w * h)) < density).astype(np.uint8) * np.uint8(one)
    return image, masks


def _run(image, masks, order, colors=None, alpha=0.5):
    out, mom = display.overlay(torch.as_tensor(image).cuda(), torch.as_tensor(masks).cuda(), order, colors, alpha)
    assert out.dtype == torch.uint8 and mom.dtype == torch.int64 and mom.is_cuda
    return out.cpu().numpy(), [tuple(int(v) for v in row) for row in mom.cpu().numpy()]


def _compare(got, want, cover, exact_up_to=16):
    """equality wherever at most `exact_up_to` painted masks cover a pixel, |diff| <= 1 elsewhere; returns the pixel counts of both branches"""
    exact = cover <= exact_up_to
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("pixels compared for equality: %d (max |diff| %d), within one grey level: %d (max |diff| %d)" %
          (exact.sum(), d[exact].max() if exact.any() else 0, (~exact).sum(), d[~exact].max() if (~exact).any() else 0))
    assert (d[exact] == 0).all()
    assert (d[~exact] <= 1).all()
    return int(exact.sum()), int((~exact).sum())


@pytest.mark.parametrize("k", [0, 1, 5])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_overlay_equals_numpy(hw, k):
    h, w = hw
    image, masks = _case(h, w, 7, seed=100 * h + w)
    order = ORDER[:k]
    colors = display.sequence_colors(k)
    got, mom = _run(image, masks, order)
    want, cover = G.composite(image, masks, order, colors, 0.5)
    n_exact, n_loose = _compare(got, want, cover)
    assert n_exact == h * w and n_loose == 0                   # at most 5 masks anywhere: the equality branch is everything
    assert mom == G.moments(masks, order, h, w)
    if k == 0:
        assert got.tobytes() == image.tobytes()
    elif h * w > 64:
        assert (got != image).any()


def test_paint_order_matters():
    h, w = 37, 53
    image, _ = _case(h, w, 1, seed=5)
    masks = np.ones((2, w * h), np.uint8)
    colors = display.sequence_colors(2)
    a, _ = _run(image, masks, [0, 1])
    b, _ = _run(image, masks, [1, 0], colors)                  # same colours per paint slot, other masks: full overlap -> same picture
    c, _ = _run(image, masks, [1, 0], colors[::-1].copy())     # the masks keep their colours, the paint order is reversed
    assert (a == b).all() and (a != c).any()
    assert (a == G.composite(image, masks, [0, 1], colors, 0.5)[0]).all()
    assert (c == G.composite(image, masks, [1, 0], colors[::-1], 0.5)[0]).all()
    # two DIFFERENT overlapping masks, painted both ways with each mask's own colour
    _, masks = _case(h, w, 2, seed=6, density=0.7)
    for order, cols in (([0, 1], colors), ([1, 0], colors[::-1].copy())):
        got, mom = _run(image, masks, order, cols)
        want, cover = G.composite(image, masks, order, cols, 0.5)
        assert _compare(got, want, cover) == (h * w, 0)
        assert mom == G.moments(masks, order, h, w)
    assert (_run(image, masks, [0, 1], colors)[0] != _run(image, masks, [1, 0], colors[::-1].copy())[0]).any()


def test_more_than_16_layers_are_within_one_grey_level():
    """k = 24 on 37 x 53: the colours wrap at 20; 20 of the masks are full, so every pixel lies under more than 16"""
    h, w, k = 37, 53, 24
    image, masks = _case(h, w, k, seed=7)
    full = np.random.default_rng(8).permutation(k)[:20]
    masks[full] = 1
    order = [int(v) for v in np.random.default_rng(9).permutation(k)]
    colors = display.sequence_colors(k)
    assert (colors[20:] == colors[:4]).all()
    got, mom = _run(image, masks, order)
    want, cover = G.composite(image, masks, order, colors, 0.5)
    assert cover.min() >= 20
    n_exact, n_loose = _compare(got, want, cover)
    assert n_exact == 0 and n_loose == h * w                   # the equality branch is empty here, and only here
    assert mom == G.moments(masks, order, h, w)


@pytest.mark.parametrize("hw", [(20, 40), (32, 33), (21, 5)], ids=lambda s: "%dx%d" % s)
def test_more_masks_than_one_colour_stage(hw):
    """k = 300 records from n = 5 masks: the kernel stages 256 colours at a time.  alpha = 1 is exact at any depth (the last covering
    mask's colour), alpha = 0.5 within one grey level"""
    h, w = hw
    k = 300
    image, masks = _case(h, w, 5, seed=31, density=0.3)
    order = [int(v) for v in np.random.default_rng(32).integers(0, 5, k)]
    colors = np.random.default_rng(33).integers(0, 256, (k, 3), dtype=np.uint8)
    got, mom = _run(image, masks, order, colors, alpha=1.0)
    want = image.copy()
    m = G.unpack(masks, h, w)
    for j, row in enumerate(order):
        want[m[row]] = colors[j]
    assert (got == want).all() and (got == G.composite(image, masks, order, colors, 1.0)[0]).all()
    assert mom == G.moments(masks, order, h, w)
    got, _ = _run(image, masks, order, colors, alpha=0.5)
    want, cover = G.composite(image, masks, order, colors, 0.5)
    n_exact, n_loose = _compare(got, want, cover)
    assert n_exact + n_loose == h * w and n_loose > 0


def test_mask_values_1_and_255_are_the_same():
    h, w = 37, 53
    image, m1 = _case(h, w, 7, seed=11, one=1)
    _, m255 = _case(h, w, 7, seed=11, one=255)
    assert ((m1 != 0) == (m255 != 0)).all() and m255.max() == 255
    a, ma = _run(image, m1, ORDER)
    b, mb = _run(image, m255, ORDER)
    assert (a == b).all() and ma == mb
    assert (a == G.composite(image, m1, ORDER, display.sequence_colors(5), 0.5)[0]).all()


def test_alpha_quarter_is_exact():
    h, w = 37, 53
    image, masks = _case(h, w, 7, seed=12)
    got, _ = _run(image, masks, ORDER, alpha=0.25)
    want, cover = G.composite(image, masks, ORDER, display.sequence_colors(5), 0.25)
    assert _compare(got, want, cover, exact_up_to=8) == (h * w, 0)       # 2 fractional bits per layer: 8 + 2 * 5 bits


def test_alpha_0_and_1():
    h, w = 37, 53
    image, masks = _case(h, w, 7, seed=13)
    colors = display.sequence_colors(5)
    got, _ = _run(image, masks, ORDER, alpha=0.0)
    assert got.tobytes() == image.tobytes()
    got, _ = _run(image, masks, ORDER, alpha=1.0)
    want = image.copy()
    m = G.unpack(masks, h, w)
    for j, row in enumerate(ORDER):                            # the last covering mask's colour
        want[m[row]] = colors[j]
    assert (got == want).all()


def test_order_entry_outside_the_masks_paints_nothing():
    h, w = 37, 53
    image, masks = _case(h, w, 3, seed=14)
    order = [2, 9, -1, 0]
    colors = display.sequence_colors(4)
    got, mom = _run(image, masks, order)
    assert (got == G.composite(image, masks, order, colors, 0.5)[0]).all()
    assert mom == G.moments(masks, order, h, w) and mom[1] == (0, 0, 0) and mom[2] == (0, 0, 0)


def test_wide_image_sums_pass_2_to_the_32():
    """h = 2048, w = 4096, one full mask: the column sum is 2048 * 4095 * 4096 / 2 > 2^32"""
    h, w = 2048, 4096
    image = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    masks = torch.ones((1, w * h), dtype=torch.uint8, device="cuda")
    out, mom = display.overlay(image, masks, [0])
    want_mom = (h * w, w * h * (h - 1) // 2, h * w * (w - 1) // 2)
    assert want_mom[2] == 2048 * 4095 * 4096 // 2 and want_mom[2] > 2 ** 32
    assert tuple(int(v) for v in mom.cpu().numpy()[0]) == want_mom
    # every pixel under one layer of (0, 255, 0): v = (image + colour) / 2, out = floor(v + 0.5) = (image + colour + 1) // 2, in integers
    col = torch.tensor([0, 255, 0], dtype=torch.int32, device="cuda")
    want = ((image.to(torch.int32) + col + 1) // 2).to(torch.uint8)
    assert bool((out == want).all())


@pytest.mark.parametrize("what", ["alpha", "h", "k"])
def test_argument_errors(what):
    h, w, k = 8, 8, 2
    image = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.full_like(image, 7)
    masks = torch.ones((2, h * w), dtype=torch.uint8, device="cuda")
    order = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    colors = torch.as_tensor(display.sequence_colors(2)).cuda()
    mom = torch.full((2, 3), -5, dtype=torch.int64, device="cuda")
    alpha = 1.5 if what == "alpha" else 0.5
    if what == "h":
        h = 0
    if what == "k":
        k = -1
    L = lib()
    with pytest.raises(RsisHipError):
        check(L.rsis_overlay_masks(ptr(image), ptr(masks), 2, ptr(order), ptr(colors), k, alpha, ptr(out), h, w, stream()), "rsis_overlay_masks")
    if what != "alpha":
        with pytest.raises(RsisHipError):
            check(L.rsis_overlay_moments(ptr(masks), 2, ptr(order), k, h, w, ptr(mom), stream()), "rsis_overlay_moments")
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((mom == -5).all())   # nothing was launched: the outputs are untouched
    if what == "alpha":
        with pytest.raises(RsisHipError):
            display.overlay(image, masks, [0, 1], alpha=1.5)
        with pytest.raises(RsisHipError):
            display.overlay(image, masks, [0, 1], alpha=float("nan"))
    with pytest.raises(RsisHipError):                           # out may not alias image
        check(L.rsis_overlay_masks(ptr(image), ptr(masks), 2, ptr(order), ptr(colors), 2, 0.5, ptr(image), 8, 8, stream()), "rsis_overlay_masks")
    with pytest.raises(RsisHipError):                           # null pointers with k > 0
        check(L.rsis_overlay_masks(ptr(image), None, 2, ptr(order), ptr(colors), 2, 0.5, ptr(out), 8, 8, stream()), "rsis_overlay_masks")


def _decode_rle(seg):
    """COCO RLE dict (counts: bytes or str) -> (h, w) uint8"""
    from rsis_amd.cocoeval import rle_from_string
    h, w = int(seg["size"][0]), int(seg["size"][1])
    counts = rle_from_string(seg["counts"])
    vals = np.arange(len(counts), dtype=np.uint8) & 1
    return np.ascontiguousarray(np.repeat(vals, counts.astype(np.int64)).reshape(w, h).T)


def test_encode_masks_want_masks():
    from rsis_amd.eval_post import encode_masks
    r = np.random.default_rng(21)
    n, h, w = 3, 21, 30
    prob = torch.as_tensor(r.random((n, 16, 16), dtype=np.float32)).cuda()
    ignore = (r.random((h, w)) < 0.3).astype(np.uint8)
    plain = encode_masks(prob, h, w, 0.5, ignore)
    assert len(plain) == 3                                      # a default call returns what it returned before
    res = encode_masks(prob, h, w, 0.5, ignore, want_masks=True)
    assert len(res) == 4
    segs, areas, raws, (seg_d, raw_d) = res
    assert segs == plain[0] and (areas == plain[1]).all() and raws == plain[2]
    assert seg_d.is_cuda and seg_d.dtype == torch.uint8 and tuple(seg_d.shape) == (n, w * h) and tuple(raw_d.shape) == (n, w * h)
    seg_h, raw_h = G.unpack(seg_d.cpu().numpy(), h, w), G.unpack(raw_d.cpu().numpy(), h, w)
    for i in range(n):
        assert (_decode_rle(segs[i]) == seg_h[i]).all() and (_decode_rle(raws[i]) == raw_h[i]).all()
        assert int(seg_h[i].sum()) == int(areas[i])
    assert (raw_h != seg_h).any()                               # the ignore pixels are in raw only
    with_bits = encode_masks(prob, h, w, 0.5, ignore, want_bits=True, want_masks=True)
    assert len(with_bits) == 5 and with_bits[4][0].data_ptr() != 0 and len(encode_masks(prob, h, w, 0.5, ignore, want_bits=True)) == 4
    # without an ignore mask there is no separate raw copy: raw is seg
    s2, _a2, r2, (seg2, raw2) = encode_masks(prob, h, w, 0.5, None, want_masks=True)
    assert raw2 is seg2 and s2 == r2


# ------------------------------------------------------------------------------------------------------------------------------------
# python -m rsis_amd.eval --display
# ------------------------------------------------------------------------------------------------------------------------------------
CLI = ["--synthetic", "--display", "--no_display_text", "--no_run_coco_eval", "-imsize", "64", "-batch_size", "2", "-maxseqlen", "3",
       "-stop_th", "0", "-class_th", "0", "-min_size", "0"]


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _plain_synthetic_images(a):
    """the de-normalised inputs of a --synthetic run, in sample order"""
    from rsis_amd.synthetic import SyntheticLoader
    loader = SyntheticLoader(a, max(1, a.synthetic_batches // 4), a.seed + 7)
    return [display.denormalize(x[s]).cpu().numpy() for x, *_ in loader for s in range(x.shape[0])]


def _calibrate(ev):
    """Randomly initialised weights put every mask probability just below -mask_th (0.44 .. 0.50 on these inputs): every mask is empty and a
    figure shows nothing.  Shift conv_out's bias so that the median mask logit of the first batch is 0 -- about half of the pixels set."""
    from rsis_amd import ops
    from rsis_amd.test import test
    x = list(ev.loader)[0][0]
    logits = test(ev.args, ev.encoder, ev.decoder, torch.cat([x, x]) if x.size(0) == 1 else x, return_logits=True)[0]
    with torch.no_grad():
        ev.decoder.conv_out.bias -= logits.median()
    ops.bump_weight_epoch()


def _store_checkpoint(ev, a):
    """the five files of utils.save_checkpoint for the modules of `ev`"""
    import pickle
    d = os.path.join(a.models_root, a.model_name)
    os.makedirs(d, exist_ok=True)
    torch.save(ev.encoder.state_dict(), os.path.join(d, "encoder.pt"))
    torch.save(ev.decoder.state_dict(), os.path.join(d, "decoder.pt"))
    torch.save({}, os.path.join(d, "enc_opt.pt"))
    torch.save({}, os.path.join(d, "dec_opt.pt"))
    with open(os.path.join(d, "args.pkl"), "wb") as f:
        pickle.dump(a, f)


def test_eval_display_cli(tmp_path):
    """`python -m rsis_amd.eval --synthetic --display` as a child process, on a stored checkpoint whose masks are not empty (`_calibrate`)"""
    from rsis_amd.args import get_parser
    from rsis_amd.eval import Evaluate
    argv = CLI + ["-models_root", str(tmp_path), "-model_name", "disp"]
    a0 = get_parser().parse_args(argv)
    torch.manual_seed(0)
    ev = Evaluate(a0)
    _calibrate(ev)
    _store_checkpoint(ev, a0)
    del ev
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "rsis_amd.eval"] + argv, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    a = get_parser().parse_args(argv)
    figs = os.path.join(str(tmp_path), "disp", "disp_figs_%s" % a.eval_split)
    plain = _plain_synthetic_images(a)
    assert sorted(os.listdir(figs)) == ["synthetic_%06d.png" % i for i in range(len(plain))]
    differ = 0
    for i, img in enumerate(plain):
        fig = _png(os.path.join(figs, "synthetic_%06d.png" % i))
        assert fig.shape == (64, 64, 3)
        differ += int((fig != img).any())
    assert differ >= 1


def _evaluate(tmp_path, name, *extra):
    from rsis_amd.args import get_parser
    from rsis_amd.eval import Evaluate
    a = get_parser().parse_args(["-models_root", str(tmp_path), "-model_name", name, "-hidden_size", "32", "-num_workers", "2"] + list(extra))
    torch.manual_seed(0)
    ev = Evaluate(a)
    _calibrate(ev)
    ev.run_eval()
    return a, ev


def test_save_figure_equals_the_numpy_composite(tmp_path):
    a, ev = _evaluate(tmp_path, "inproc", *CLI, "-synthetic_batches", "4")
    plain = _plain_synthetic_images(a)
    assert len(ev.figures) == len(plain) == 2
    checked = 0
    for (path, records, rects), img in zip(ev.figures, plain):
        assert rects == [] and len(records) > 0
        masks = G.pack(np.stack([_decode_rle(r["segmentation"]) for r in records]))
        colors = display.sequence_colors(len(records))
        want, cover = G.composite(img, masks, range(len(records)), colors, 0.5)
        assert cover.max() <= 16
        assert (_png(path) == want).all()
        checked += int((want != img).any())
    assert checked >= 1
    # text on: the same composite everywhere outside the label rectangles save_figure reports, and something else inside at least one
    path, records, _ = ev.figures[0]
    assert [r["mask_row"] for r in records] == [0, 1, 2]
    recs = [dict(r, mask_row=i) for i, r in enumerate(records)]
    out = str(tmp_path / "text.png")
    rects = display.save_figure(out, torch.as_tensor(plain[0]).cuda(), torch.as_tensor(masks_of(records)).cuda(), recs)
    want = _png(path)
    got = _png(out)
    assert len(rects) >= 1
    inside = np.zeros(got.shape[:2], bool)
    for x0, y0, x1, y1 in rects:
        inside[y0:y1, x0:x1] = True
    assert (got[~inside] == want[~inside]).all()
    assert any((got[y0:y1, x0:x1] != want[y0:y1, x0:x1]).any() for x0, y0, x1, y1 in rects)
    # --display_route: indices as labels and a red line through the anchors; still the composite away from the labels and the line
    out2 = str(tmp_path / "route.png")
    display.save_figure(out2, torch.as_tensor(plain[0]).cuda(), torch.as_tensor(masks_of(records)).cuda(), recs, display_route=True)
    assert _png(out2).shape == want.shape


def masks_of(records):
    return G.pack(np.stack([_decode_rle(r["segmentation"]) for r in records]))


def test_no_display_no_figures(tmp_path):
    argv = [v for v in CLI if v != "--display"] + ["-synthetic_batches", "4"]
    a, ev = _evaluate(tmp_path, "plainrun", *argv)
    assert ev.figures == []
    assert sorted(os.listdir(os.path.join(str(tmp_path), "plainrun"))) == ["plainrun_%s_predictions.json" % a.eval_split]


def test_eval_display_cityscapes_tree(tmp_path):
    """-dataset cityscapes in rsis_amd.eval: one figure per image, named after the file, at the image's ORIGINAL size"""
    from rsis_amd.dataloader.cityscapes import synthesize_cityscapes_dir
    synthesize_cityscapes_dir(str(tmp_path / "city"), n=2, sizes=((40, 72), (64, 128)))
    a, ev = _evaluate(tmp_path, "city", "-dataset", "cityscapes", "-cityscapes_dir", str(tmp_path / "city"), "-eval_split", "val",
                      "-num_classes", "9", "-imsize", "32", "--resize", "-batch_size", "2", "-maxseqlen", "3", "-stop_th", "0",
                      "-class_th", "0", "-min_size", "0", "--display")
    figs = os.path.join(str(tmp_path), "city", "city_figs_val")
    files = ev.dataset.get_sample_list()
    assert len(files) == 2
    assert sorted(os.listdir(figs)) == sorted(os.path.basename(f) for f in files)
    for f, (path, records, _rects) in zip(files, ev.figures):
        plain = _png(f)
        fig = _png(path)
        assert fig.shape == plain.shape and os.path.basename(path) == os.path.basename(f)
        masks = masks_of(records)
        want, _ = G.composite(plain, masks, range(len(records)), display.sequence_colors(len(records)), 0.5)
        assert (fig[~_labelled(_rects, fig)] == want[~_labelled(_rects, fig)]).all() and (want != plain).any()
        assert all(r["category_name"] in ev.class_names[1:] for r in records)
    assert {tuple(_png(p).shape[:2]) for p, _, _ in ev.figures} == {(40, 72), (64, 128)}
    assert not os.path.exists(os.path.join(str(tmp_path), "city", "city_val_cocoeval.json"))     # no ground truth: not evaluated
    assert os.path.exists(os.path.join(str(tmp_path), "city", "city_val_predictions.json"))


def _labelled(rects, fig):
    inside = np.zeros(fig.shape[:2], bool)
    for x0, y0, x1, y1 in rects:
        inside[y0:y1, x0:x1] = True
    return inside


def test_eval_display_leaves_tree(tmp_path):
    """-dataset leaves: every record of a timestep whose objectness exceeds -stop_th is drawn (eval.py:329-331)"""
    from rsis_amd.dataloader.leaves import synthesize_leaves_dir
    d = synthesize_leaves_dir(str(tmp_path / "A1"), n=4, size=(48, 56))
    a, ev = _evaluate(tmp_path, "leaf", "-dataset", "leaves", "-leaves_test_dir", d, "-eval_split", "test", "-num_classes", "2",
                      "-imsize", "32", "--resize", "-batch_size", "2", "-maxseqlen", "3", "-stop_th", "0", "-class_th", "0",
                      "-min_size", "0", "--display", "--no_display_text")
    figs = os.path.join(str(tmp_path), "leaf", "leaf_figs_test")
    assert sorted(os.listdir(figs)) == ["plant%03d_rgb.png" % i for i in range(4)]
    for f, (path, records, rects) in zip(ev.dataset.get_sample_list(), ev.figures):
        plain = _png(f)
        assert plain.shape == (48, 56, 3) and rects == []
        assert len(records) == 3 and [r["mask_row"] for r in records] == [0, 1, 2]   # one class: one record per timestep
        want, _ = G.composite(plain, masks_of(records), range(3), display.sequence_colors(3), 0.5)
        assert (_png(path) == want).all() and (want != plain).any()


def test_eval_display_pascal_tree(tmp_path):
    """-dataset pascal: figures named after the sample ids, the JPEG as background, the RAW masks (before the ignore pixels) on top"""
    from rsis_amd import pascal_precompute
    from rsis_amd.dataloader.pascal import synthesize_pascal_dir
    d = synthesize_pascal_dir(str(tmp_path / "VOC"), n=5, sizes=((64, 80), (50, 70)), seed=8)
    pascal_precompute.run(d, "val", verbose=False)
    a, ev = _evaluate(tmp_path, "voc", "-dataset", "pascal", "-pascal_dir", d, "-eval_split", "val", "-batch_size", "2", "--resize", "-imsize", "64",
                      "-maxseqlen", "3", "-stop_th", "0", "-class_th", "0", "-min_size", "0", "--no_run_coco_eval", "--display",
                      "--no_display_text")
    figs = os.path.join(str(tmp_path), "voc", "voc_figs_val")
    assert sorted(os.listdir(figs)) == sorted(n + ".png" for n in ev.sample_list) and len(ev.figures) == len(ev.sample_list) == 2
    for i, (path, records, rects) in enumerate(ev.figures):
        plain = _png(ev.dataset.image_path(i))
        assert plain.shape[:2] == tuple(ev.dataset.raw_size(i)) and len(records) == 3 and rects == []
        want, _ = G.composite(plain, masks_of(records), range(3), display.sequence_colors(3), 0.5)
        assert (_png(path) == want).all() and (want != plain).any()
