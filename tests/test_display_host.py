"""CPU tests of the --display path (rsis_amd/display.py, the eval.py wiring): the numpy statement of the compositing
(tests/overlay_golden.py) against a case computed by hand, the colour table, the label text and anchor arithmetic of reference
eval.py:53-74, the figure file names of eval.py:353-358 and the command-line flags.  No kernel runs here: tests/test_gpu_display.py."""
import numpy as np
import pytest

import overlay_golden as G
from rsis_amd import display
from rsis_amd.args import get_parser

GREEN, RED = (0, 255, 0), (255, 0, 0)
# h = 2, w = 3
IMAGE = np.array([[(10, 20, 30), (100, 101, 102), (255, 0, 7)],
                  [(0, 0, 0), (200, 50, 25), (9, 8, 7)]], np.uint8)
MASK_A = np.array([[1, 1, 0],
                   [0, 1, 0]], np.uint8)
MASK_B = np.array([[0, 1, 0],
                   [0, 1, 1]], np.uint8)


def test_numpy_statement_on_a_case_computed_by_hand():
    masks = G.pack(np.stack([MASK_A, MASK_B]))
    assert masks.tolist() == [[1, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 1]]              # column-major: element x * h + y
    out, cover = G.composite(IMAGE, masks, [0, 1], [GREEN, RED], 0.5)
    # (0,0): A only: (10+0)/2, (20+255)/2 = 137.5 -> 138, (30+0)/2
    # (0,1): A: (50, 178, 51), then B: (152.5, 89, 25.5) -> (153, 89, 26)
    # (1,1): A: (100, 152.5, 12.5), then B: (177.5, 76.25, 6.25) -> (178, 76, 6)
    # (1,2): B only: (132, 4, 3.5 -> 4)
    want = np.array([[(5, 138, 15), (153, 89, 26), (255, 0, 7)],
                     [(0, 0, 0), (178, 76, 6), (132, 4, 4)]], np.uint8)
    assert out.tolist() == want.tolist()
    assert cover.tolist() == [[1, 2, 0], [0, 2, 1]]
    # the other paint order: (0,1): B: (177.5, 50.5, 51), then A: (88.75, 152.75, 25.5) -> (89, 153, 26)
    rev, _ = G.composite(IMAGE, masks, [1, 0], [RED, GREEN], 0.5)
    assert rev[0, 1].tolist() == [89, 153, 26] and rev[0, 0].tolist() == [5, 138, 15]
    # an entry outside [0, n) paints nothing; k = 0 is the image
    assert G.composite(IMAGE, masks, [7], [RED], 0.5)[0].tolist() == IMAGE.tolist()
    assert G.composite(IMAGE, masks, [], [], 0.5)[0].tolist() == IMAGE.tolist()
    # A: pixels (y, x) = (0,0) (0,1) (1,1); B: (0,1) (1,1) (1,2)
    assert G.moments(masks, [0, 1, 5], 2, 3) == [(3, 1, 2), (3, 2, 4), (0, 0, 0)]


def test_sequence_colors_are_the_reference_palette_ids_1_to_20():
    want = [(0, 255, 0), (255, 0, 0), (0, 0, 255), (255, 0, 255), (0, 255, 255), (255, 128, 0), (102, 0, 102), (51, 153, 255),
            (153, 153, 255), (153, 153, 0), (178, 102, 255), (204, 0, 204), (0, 102, 0), (102, 0, 0), (51, 0, 0), (0, 64, 0),
            (128, 64, 0), (0, 192, 0), (128, 192, 0), (0, 64, 128)]
    assert [tuple(c) for c in display.SEQUENCE_COLORS] == want
    c = display.sequence_colors(23)                                                # the i-th drawn record gets colour i % 20
    assert c.dtype == np.uint8 and c.shape == (23, 3)
    assert [tuple(int(v) for v in r) for r in c] == want + want[:3]
    assert display.sequence_colors(0).shape == (0, 3)


@pytest.mark.parametrize("name,shown", [("motorbike", "motor"), ("bicycle", "bike"), ("dining table", "table"),
                                        ("potted plant", "plant"), ("airplane", "plane"), ("person", "person")])
def test_display_name(name, shown):
    assert display.display_name(name) == shown


def _pixel(cy, cx):
    return (1, cy, cx)                                                             # the moments of a one-pixel mask


def test_label_anchors_clamps():
    h, w = 100, 200
    mom = [_pixel(50, 100),          # no clamp: (100 - 30, 50 - 10)
           _pixel(50, 10),           # x - 30 < 0 -> 0
           _pixel(5, 100),           # y - 10 < 0 -> 0
           (0, 0, 0),                # an empty mask gets no label
           (4, 2 * 99 + 2 * 98, 2 * 199 + 2 * 198)]   # the bottom-right 2 x 2 pixels: centre (98.5, 198.5)
    got = display.label_anchors(np.asarray(mom, np.int64), h, w)
    assert got == [(70.0, 40.0), (0.0, 40.0), (70.0, 0.0), None, (168.5, 88.5)]
    assert got == G.anchors(mom, h, w)
    # an image smaller than the 30 x 10 box: max(0, .) first, then min(h - 10, .) / min(w - 30, .) as the reference orders them
    small = display.label_anchors([_pixel(3, 10)], 6, 20)
    assert small == [(-10.0, -4.0)] and small == G.anchors([_pixel(3, 10)], 6, 20)
    # only one of the two upper clamps bites: 45 x 25
    assert display.label_anchors([_pixel(20, 40)], 25, 45) == [(10.0, 10.0)]
    assert display.label_anchors([_pixel(24, 44)], 25, 45) == [(14.0, 14.0)]
    assert display.label_anchors([_pixel(24, 44)], 25, 35) == [(5.0, 14.0)]      # w - 30 = 5 < 14
    assert display.label_anchors([_pixel(24, 44)], 15, 45) == [(14.0, 5.0)]      # h - 10 = 5 < 14
    # sums beyond 2^32 (2048 x 4096, a full mask) stay exact
    hh, ww = 2048, 4096
    full = (hh * ww, ww * hh * (hh - 1) // 2, hh * ww * (ww - 1) // 2)
    assert display.label_anchors([full], hh, ww) == [(2047.5 - 30, 1023.5 - 10)]


def test_figure_file_names():
    assert display.figure_name("2007_000033", "pascal") == "2007_000033.png"
    assert display.figure_name("synthetic_000004") == "synthetic_000004.png"
    city = "/data/CityScapes/leftImg8bit/val/frankfurt/frankfurt_000000_000294_leftImg8bit"
    assert display.figure_name(city, "cityscapes") == "frankfurt_000000_000294_leftImg8bit.png"
    assert display.figure_name(city + ".png", "cityscapes") == "frankfurt_000000_000294_leftImg8bit.png"
    assert display.figure_name("/data/LeavesDataset/A1/plant001_rgb.png", "leaves") == "plant001_rgb.png"
    import os
    assert display.figures_dir("../models", "m", "val") == os.path.join("../models", "m", "m_figs_val")


def test_display_flags_parse():
    p = get_parser()
    a = p.parse_args([])
    assert (a.display, a.no_display_text, a.display_route) == (False, False, False)
    a = p.parse_args(["--display", "--no_display_text", "--display_route", "-dataset", "leaves"])
    assert (a.display, a.no_display_text, a.display_route, a.dataset) == (True, True, True, "leaves")


def test_draw_labels_reports_the_rectangles_it_touches():
    """host part of save_figure: the boxes and texts change pixels only inside the rectangles it returns"""
    rgb = np.full((40, 90, 3), 200, np.uint8)
    before = rgb.copy()
    rects = display.draw_labels(rgb, [(5.0, 4.0), None, (60.0, 25.0)], ["motor", "bike", "7"], display.sequence_colors(3))
    assert len(rects) == 2
    inside = np.zeros(rgb.shape[:2], bool)
    for x0, y0, x1, y1 in rects:
        assert 0 <= x0 < x1 <= 90 and 0 <= y0 < y1 <= 40
        inside[y0:y1, x0:x1] = True
    assert (rgb[~inside] == before[~inside]).all()
    for x0, y0, x1, y1 in rects:
        assert (rgb[y0:y1, x0:x1] != before[y0:y1, x0:x1]).any()
    # the box is the record's colour at opacity 0.6 over the image: green over 200 -> (80, 233, 80) wherever no text lies
    x0, y0, x1, y1 = rects[0]
    assert rgb[y0, x0].tolist() == [80, 233, 80]
