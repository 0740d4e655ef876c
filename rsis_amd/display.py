"""Figures of `eval --display` -- counterpart of reference src/eval.py:30-95 `display_masks` and :342-359: one figure per image, the image
with every kept instance mask painted over it in its sequence colour at opacity 0.5 and the class name at the mask's centre of mass.

The compositing runs in librsis_hip.so (overlay.hip: rsis_overlay_masks / rsis_overlay_moments) on the byte masks that
rsis_mask_resize_threshold left on the device; ONE copy of the finished h x w x 3 image comes back to the host, where PIL writes the
few labels and the PNG.  No matplotlib is involved, and a figure is NOT pixel-identical to the reference's and does not claim to be:
matplotlib resamples the image to the figure's dpi and crops it with `bbox_inches='tight'`, its text is rendered by another rasteriser
with another font; here the figure has the image's own resolution, the font is `ImageFont.load_default()` and a label's top-left corner
sits at the anchor.  What is restated exactly: the blend (`ax.imshow` of an RGBA layer with alpha 0.5 per mask, in record order), the
colours, the label anchor arithmetic (display_masks:70-74), the abbreviations (:53-63), the 0.6-opaque box in the mask's colour behind
the text, labels after all masks, the red 1-pixel route of --display_route.

Deliberate difference: the i-th drawn record gets colour `i % 20` -- the reference indexes its 20 colours with i and raises IndexError
at the 21st record of an image.  An empty mask gets no label (the reference's centre of mass is NaN there)."""
import numpy as np
import torch

from ._lib import RsisHipError, check, lib, ptr, stream

# reference dataloader/dataset_utils.py sequence_palette() ids 1 .. 20 in id order (eval.py:221-231 drops 0 and 21)
SEQUENCE_COLORS = ((0, 255, 0), (255, 0, 0), (0, 0, 255), (255, 0, 255), (0, 255, 255), (255, 128, 0), (102, 0, 102), (51, 153, 255),
                   (153, 153, 255), (153, 153, 0), (178, 102, 255), (204, 0, 204), (0, 102, 0), (102, 0, 0), (51, 0, 0), (0, 64, 0),
                   (128, 64, 0), (0, 192, 0), (128, 192, 0), (0, 64, 128))
MASK_ALPHA = 0.5                 # display_masks:83
BOX_ALPHA = 0.6                  # display_masks:87
BOX_WIDTH, BOX_HEIGHT = 30, 10   # display_masks:36-37
BOX_PAD = 2                      # pixels of box around the text
_ABBREVIATIONS = {"motorbike": "motor", "bicycle": "bike", "dining table": "table", "potted plant": "plant", "airplane": "plane"}
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # eval.py:185


def sequence_colors(k):
    """(k, 3) uint8 array: colour i % 20 for the i-th drawn record"""
    return np.asarray([SEQUENCE_COLORS[i % len(SEQUENCE_COLORS)] for i in range(k)], dtype=np.uint8).reshape(k, 3)


def display_name(category_name):
    """display_masks:53-63"""
    return _ABBREVIATIONS.get(category_name, category_name)


def figure_name(sample_idx, dataset=None):
    """file name of an image's figure (eval.py:353-358): the sample id for Pascal and synthetic runs, the file's basename without its
    extension for Cityscapes and leaves, whose sample ids are paths"""
    name = str(sample_idx)
    if dataset in ("cityscapes", "leaves"):
        name = name.split("/")[-1].split(".")[0]
    return name + ".png"


def figures_dir(models_root, model_name, eval_split):
    import os
    return os.path.join(models_root, model_name, "%s_figs_%s" % (model_name, eval_split))


def overlay(image_u8, masks, order, colors=None, alpha=MASK_ALPHA):
    """image_u8: (h, w, 3) CUDA uint8 RGB; masks: CUDA uint8, n COLUMN-major h x w masks ((n, w * h) or (n, w, h): the seg / raw layout
    of rsis_mask_resize_threshold), zero / non-zero; order: the mask rows to paint, in paint order (ints, or an int32 CUDA tensor);
    colors: (k, 3) uint8, default `sequence_colors(k)` -> (out (h, w, 3) CUDA uint8, moments (k, 3) CUDA int64: set pixels, sum of row
    indices, sum of column indices of each painted mask).  Nothing is copied to the host."""
    if not (torch.is_tensor(image_u8) and image_u8.is_cuda and image_u8.dtype == torch.uint8 and image_u8.dim() == 3 and image_u8.size(2) == 3):
        raise RsisHipError("overlay: image must be a CUDA uint8 tensor of shape (h, w, 3); there is no CPU path")
    if not (torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() in (2, 3)):
        raise RsisHipError("overlay: masks must be a CUDA uint8 tensor of n column-major masks")
    dev = image_u8.device
    image_u8, masks = image_u8.contiguous(), masks.contiguous()
    h, w = int(image_u8.size(0)), int(image_u8.size(1))
    n = int(masks.size(0))
    if n and masks.numel() != n * h * w:
        raise ValueError("overlay: %d masks of %d elements do not fit a %d x %d image" % (n, masks.numel() // n, h, w))
    if torch.is_tensor(order):
        order = order.to(device=dev, dtype=torch.int32).contiguous()
    else:
        order = torch.as_tensor([int(v) for v in order], dtype=torch.int32).to(dev)
    k = int(order.numel())
    if colors is None:
        colors = sequence_colors(k)
    if not torch.is_tensor(colors):
        colors = torch.as_tensor(np.ascontiguousarray(np.asarray(colors, dtype=np.uint8).reshape(k, 3)))
    colors = colors.to(device=dev, dtype=torch.uint8).contiguous()
    if colors.numel() != 3 * k:
        raise ValueError("overlay: %d colours for %d masks" % (colors.numel() // 3, k))
    out = torch.empty_like(image_u8)
    moments = torch.zeros((k, 3), dtype=torch.int64, device=dev)
    L = lib()
    check(L.rsis_overlay_masks(ptr(image_u8), ptr(masks) if n else None, n, ptr(order) if k else None, ptr(colors) if k else None, k,
                               float(alpha), ptr(out), h, w, stream()), "rsis_overlay_masks")
    check(L.rsis_overlay_moments(ptr(masks) if n else None, n, ptr(order) if k else None, k, h, w, ptr(moments) if k else None, stream()),
          "rsis_overlay_moments")
    return out, moments


def label_anchors(moments, h, w):
    """moments: (k, 3) integers (set pixels, sum of row indices, sum of column indices) -> list of k label anchors (x, y) in float64, or
    None for an empty mask.  display_masks:70-74: the centre of mass, moved up-left by the box and clamped in the reference's order
    (an image smaller than the box ends at negative coordinates, as there)."""
    if torch.is_tensor(moments):
        moments = moments.cpu().numpy()
    m = np.asarray(moments).reshape(-1, 3)
    out = []
    for area, srow, scol in m:
        if int(area) <= 0:
            out.append(None)
            continue
        y, x = float(int(srow)) / float(int(area)), float(int(scol)) / float(int(area))
        x = max(0, x - BOX_WIDTH)
        y = max(0, y - BOX_HEIGHT)
        y = min(h - BOX_HEIGHT, y)
        x = min(w - BOX_WIDTH, x)
        out.append((float(x), float(y)))
    return out


def denormalize(x):
    """(3, H, W) CUDA image normalised with the ImageNet mean / std (eval.py:185) -> (H, W, 3) uint8 on the device"""
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=x.device).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=x.device).view(3, 1, 1)
    v = ((x.detach().float() * std + mean) * 255.0).clamp(0.0, 255.0).round()
    return v.permute(1, 2, 0).contiguous().to(torch.uint8)


def draw_labels(rgb, anchors, texts, colors, route=False):
    """rgb: (h, w, 3) uint8 host array (changed in place): per anchor that is not None a box in the record's colour at opacity 0.6 with the
    text on it, then with `route` a red 1-pixel polyline through the anchors.  Returns the label rectangles (x0, y0, x1, y1), half open
    and clipped to the image, in record order (an empty list entry is never made: records without a label are skipped)."""
    from PIL import Image, ImageDraw, ImageFont
    h, w = rgb.shape[:2]
    font = ImageFont.load_default()
    probe = ImageDraw.Draw(Image.new("RGB", (1, 1)))
    rects, jobs = [], []
    for a, text, col in zip(anchors, texts, colors):
        if a is None or text is None:
            continue
        px, py = int(round(a[0])), int(round(a[1]))
        l, t, r, b = probe.textbbox((px, py), text, font=font)
        x0, y0, x1, y1 = max(0, min(px, l) - BOX_PAD), max(0, min(py, t) - BOX_PAD), min(w, r + BOX_PAD), min(h, b + BOX_PAD)
        if x1 <= x0 or y1 <= y0:
            continue
        box = rgb[y0:y1, x0:x1].astype(np.float64)
        rgb[y0:y1, x0:x1] = np.floor(box + BOX_ALPHA * (np.asarray(col, np.float64) - box) + 0.5).astype(np.uint8)
        rects.append((x0, y0, x1, y1))
        jobs.append((px, py, text))
    im = Image.fromarray(rgb)
    draw = ImageDraw.Draw(im)
    for px, py, text in jobs:
        draw.text((px, py), text, fill=(0, 0, 0), font=font)
    if route:
        pts = [(int(round(a[0])), int(round(a[1]))) for a in anchors if a is not None]
        if len(pts) > 1:
            draw.line(pts, fill=(255, 0, 0), width=1)
    rgb[...] = np.asarray(im)
    return rects


def save_figure(path, image_u8, masks, records, no_display_text=False, display_route=False):
    """Write the figure of one image as a PNG of the image's own resolution.  image_u8: (h, w, 3) CUDA uint8; masks: the image's
    column-major byte masks on the device (`overlay`); records: the records to draw, in order -- dicts with `mask_row` (the row of
    `masks`) and `category_name`.  The masks are composited on the device, the result is copied to the host once, then the labels --
    the display name, or the record's index with display_route -- are drawn with PIL, all of them after all masks.  Returns the label
    rectangles (`draw_labels`; [] with no_display_text)."""
    from PIL import Image
    k = len(records)
    h, w = int(image_u8.size(0)), int(image_u8.size(1))
    colors = sequence_colors(k)
    out, moments = overlay(image_u8, masks, [int(r["mask_row"]) for r in records], colors)
    want_anchors = k > 0 and (display_route or not no_display_text)
    anchors = label_anchors(moments, h, w) if want_anchors else [None] * k
    rgb = np.ascontiguousarray(out.cpu().numpy())                       # the one copy of the h x w x 3 result
    rects = []
    if want_anchors:
        if no_display_text:
            texts = [None] * k
        elif display_route:
            texts = ["%d" % i for i in range(k)]
        else:
            texts = [display_name(r["category_name"]) for r in records]
        rects = draw_labels(rgb, anchors, texts, colors, route=display_route)
    Image.fromarray(rgb).save(path, format="PNG")
    return rects
