"""float64 numpy statement of the --display compositing (rsis_overlay_masks / rsis_overlay_moments, rsis_amd/display.py), written from
the definitions and not from the kernels.  Masks come as the device has them: n COLUMN-major h x w byte masks, element x * h + y, zero /
non-zero.

composite : v = image; for j = 0 .. k-1 in order, where mask order[j] is non-zero: v = v + alpha * (colors[j] - v); out = floor(v + 0.5).
            Also returns, per pixel, how many painted masks cover it.  In float64 this is EXACT for every alpha = 2^-b whose layers stay
            within 53 bits (alpha 0.5: 44 layers over an 8-bit value), so it states the real-number result; the device's fp32 fmaf chain is
            exact, too, while 8 + b * (covering masks) <= 24 bits.
moments   : (set pixels, sum of row indices, sum of column indices) per painted mask, python integers.
anchors   : reference eval.py display_masks lines 70-74 on those moments; None for an empty mask.
An order entry outside [0, n) paints nothing and has zero moments."""
import numpy as np

BOX_WIDTH, BOX_HEIGHT = 30, 10


def unpack(masks_cm, h, w):
    """(n, w * h) column-major bytes -> (n, h, w) bool"""
    m = np.asarray(masks_cm)
    n = m.shape[0]
    return m.reshape(n, w, h).transpose(0, 2, 1) != 0


def pack(masks_hw):
    """(n, h, w) array -> (n, w * h) column-major uint8 with the same values"""
    m = np.asarray(masks_hw)
    return np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(m.shape[0], -1).astype(np.uint8)


def composite(image, masks_cm, order, colors, alpha):
    image = np.asarray(image)
    h, w = image.shape[:2]
    m = unpack(masks_cm, h, w) if len(masks_cm) else np.zeros((0, h, w), bool)
    v = image.astype(np.float64)
    cover = np.zeros((h, w), np.int64)
    for j, row in enumerate(order):
        if not 0 <= int(row) < m.shape[0]:
            continue
        on = m[int(row)]
        c = np.asarray(colors[j], np.float64)
        v[on] = v[on] + np.float64(alpha) * (c - v[on])
        cover += on
    return np.floor(v + 0.5).astype(np.uint8), cover


def moments(masks_cm, order, h, w):
    m = unpack(masks_cm, h, w) if len(masks_cm) else np.zeros((0, h, w), bool)
    out = []
    for row in order:
        if not 0 <= int(row) < m.shape[0]:
            out.append((0, 0, 0))
            continue
        ys, xs = np.nonzero(m[int(row)])
        out.append((int(ys.size), int(ys.astype(np.int64).sum()), int(xs.astype(np.int64).sum())))
    return out


def anchors(mom, h, w):
    out = []
    for area, srow, scol in mom:
        if area == 0:
            out.append(None)
            continue
        y, x = np.float64(srow) / np.float64(area), np.float64(scol) / np.float64(area)
        x = max(0, x - BOX_WIDTH)
        y = max(0, y - BOX_HEIGHT)
        y = min(h - BOX_HEIGHT, y)
        x = min(w - BOX_WIDTH, x)
        out.append((float(x), float(y)))
    return out
