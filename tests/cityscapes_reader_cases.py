"""Shared by the Cityscapes reader tests: the two numpy statements of the label work and the case builders.

reference_raw_sample : what the reference's reader computes from a `*_instanceIds` image at full resolution (its lines 67-92, with the
                       python-2 `/` on integers written `//`): the class map by label arithmetic, the instance map by np.unique and one
                       compare per instance.  Defined for the values the dataset holds: below 1000, or label 24..33.
device_rule          : the rule of rsis_instance_maps (include/rsis_hip.h) in numpy.

Run as a script, this file checks on the CPU -- for id images at 64x128 -> 16x32, 64x128 -> 24x48, 96x200 -> 25x52 and
1024x2048 -> 256x512 -- that `sequence_from_masks` of (reference compaction, then the nearest zoom of both maps) equals
`sequence_from_masks` of (nearest zoom of the raw ids, then the device rule), including instances that vanish under the sampling.
tests/test_cityscapes_reader_host.py runs the three small sizes."""
import numpy as np

LABELS = (24, 25, 26, 27, 28, 29, 30, 31, 32, 33)
TABLE = [0] * 24 + [1, 2, 3, 4, 5, 0, 0, 6, 7, 8]              # what rsis_amd.dataloader.cityscapes.CLASS_OF_LABEL must equal
CUSTOM_TABLE = [0, 3] + [0] * 63 + [2]                          # label 1 -> 3, label 65 -> 2: raw 1000 and 65535 are kept
COMMUTE_SIZES = [((64, 128), (16, 32)), ((64, 128), (24, 48)), ((96, 200), (25, 52))]
FULL_SIZE = ((1024, 2048), (256, 512))


def reference_raw_sample(raw):
    """(H, W) raw ids -> (ins, seg) as the reference's get_raw_sample returns them"""
    ins = np.array(raw, dtype=np.int64)
    seg = ins // 1000
    seg[seg == 29] = 0                       # caravan and trailer are not trained
    seg[seg == 30] = 0
    seg[seg > 0] -= 23                       # classes start at 1
    seg[seg == 8] = 6                        # the three classes after the two that were dropped
    seg[seg == 9] = 7
    seg[seg == 10] = 8
    keep = (seg > 0).astype(np.int64)
    ins = ins * keep
    ins[ins < 24000] = 0
    ids = np.unique(ins)
    out = np.zeros_like(ins)
    for i, v in enumerate(ids):              # (on a copy: the reference renumbers in place, which is the same while every id exceeds every rank)
        out[ins == v] = i
    return out, seg


def defined_for_reference(raw):
    """raw with every value the reference is not defined for (outside 0..65535, or >= 1000 with a label outside 24..33) set to 0"""
    raw = np.asarray(raw, dtype=np.int64)
    label = raw // 1000
    return np.where((raw >= 1000) & ((label < 24) | (label > 33) | (raw > 65535)) | (raw < 0), 0, raw)


def device_rule(raw, table=TABLE):
    """(B, H, W) or (H, W) raw ids -> (ins, seg) int32 by the rule of rsis_instance_maps"""
    raw = np.asarray(raw, dtype=np.int64)
    single = raw.ndim == 2
    raw = raw[None] if single else raw
    tab = np.asarray(table, dtype=np.int64)
    assert 1 <= len(tab) <= 66
    raw = np.where((raw < 0) | (raw > 65535), 0, raw)
    label = raw // 1000
    seg = np.where((raw >= 1000) & (label < len(tab)), tab[np.minimum(label, len(tab) - 1)], 0)
    ins = np.zeros_like(raw)
    for b in range(raw.shape[0]):
        kept = seg[b] > 0
        present = np.unique(raw[b][kept])
        ins[b][kept] = 1 + np.searchsorted(present, raw[b][kept])
    ins, seg = ins.astype(np.int32), seg.astype(np.int32)
    return (ins[0], seg[0]) if single else (ins, seg)


def zoom_nearest(a, size):
    """the reference's resize of a label map: scipy zoom(order=0, mode='nearest') to (h, w)"""
    from scipy.ndimage import zoom
    return zoom(a, [float(size[0]) / a.shape[0], float(size[1]) / a.shape[1]], mode="nearest", order=0)


def id_image(H, W, seed, background=True):
    """an (H, W) int32 image as the dataset's: stuff bands below 1000, a group region (plain 26), overlapping rectangles and ellipses of
    all ten instance labels with two to four instances each (k from 0), a pair of equal area, and instances of one to four pixels
    that a 4x down-sampling loses.  background=False: the instances of the trained classes tile the whole image."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ids = np.zeros((H, W), np.int32)
    if not background:
        gh, gw = 4, 5
        for c in range(gh * gw):
            lab = (24, 25, 26, 27, 28, 31, 32, 33)[c % 8]
            ids[(c // gw) * H // gh:(c // gw + 1) * H // gh, (c % gw) * W // gw:(c % gw + 1) * W // gw] = lab * 1000 + c // 8
        return ids
    for j, s in enumerate((23, 11, 21, 7, 8)):
        ids[j * H // 5:(j + 1) * H // 5] = s
    ids[H // 2:H // 2 + max(2, H // 8), W // 3:W // 3 + max(2, W // 6)] = 26
    for lab in LABELS:
        for k in range(int(r.integers(2, 5))):
            cy, cx = r.uniform(0.05, 0.95) * H, r.uniform(0.05, 0.95) * W
            a, b = r.uniform(0.03, 0.12) * H + 1, r.uniform(0.03, 0.12) * W + 1
            if r.random() < 0.5:
                m = (np.abs(yy - cy) <= a) & (np.abs(xx - cx) <= b)
            else:
                m = ((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2 <= 1.0
            ids[m] = lab * 1000 + k
    e = max(2, H // 10)                                          # two squares of equal area, drawn last: nothing covers them
    ids[0:e, 0:e] = 24000 + 900
    ids[H - e:H, W - e:W] = 33000 + 900
    for t in range(6):                                           # specks
        y, x = int(r.integers(e, H - e - 1)), int(r.integers(e, W - e - 1))
        ids[y:y + 1 + t % 2, x:x + 1 + t // 3] = LABELS[t] * 1000 + 950 + t
    return ids


def targets_of(ins, seg, T):
    from rsis_amd.dataloader import sequence_from_masks
    return sequence_from_masks(ins, seg, T)


def commutation_holds(raw, size, T=20):
    """(ok, instances at full resolution, instances left after the zoom) for one id image"""
    ins, seg = reference_raw_sample(raw)
    a = targets_of(zoom_nearest(ins, size), zoom_nearest(seg, size), T)
    d_ins, d_seg = device_rule(zoom_nearest(raw, size))
    b = targets_of(d_ins, d_seg, T)
    return bool(np.array_equal(a, b)), int(ins.max()), int(d_ins.max())


# ---- the cases of the device tests: name -> (3, H, W) int32 raw ids ----
MIXED_VALUES = [lab * 1000 + k for lab in LABELS for k in (0, 999)] + [0, 7, 26, 999, 5000, 34000, 65535, -1, 70000]


def _fill(r, H, W, values):
    """(H, W) image holding EVERY value of `values`, the rest drawn from them, scattered"""
    hw = H * W
    assert len(values) <= hw
    flat = np.concatenate([np.asarray(values, np.int64), r.choice(np.asarray(values, np.int64), hw - len(values))])
    return flat[r.permutation(hw)].reshape(H, W).astype(np.int32)


def device_cases(H, W):
    r = np.random.default_rng(H * 1000 + W + 5)
    out = {}
    if H * W >= len(MIXED_VALUES):
        out["mixed"] = np.stack([_fill(r, H, W, MIXED_VALUES), _fill(r, H, W, MIXED_VALUES[:13] + [0, 7, -1]),
                                 _fill(r, H, W, MIXED_VALUES[6:])])
    none = [0, 7, 26, 999, 29000, 29999, 30001, 5000, 23999, 34000, 65535, -1, 70000, -2147483648, 2147483647]
    out["none"] = np.stack([_fill(r, H, W, none), np.zeros((H, W), np.int32), _fill(r, H, W, none[:5])])
    kept = [lab * 1000 + k for lab in (24, 25, 26, 27, 28, 31, 32, 33) for k in (0, 1, 2)]
    out["no_background"] = np.stack([_fill(r, H, W, kept), np.full((H, W), 31005, np.int32), _fill(r, H, W, kept[:2])])
    custom = [1000, 1999, 65000, 65535, 24000, 999, 0, 2000, 64999]
    out["custom"] = np.stack([_fill(r, H, W, custom), _fill(r, H, W, custom[:2]), _fill(r, H, W, custom[2:])])
    if H * W >= 96 * 112:
        dense = [24000 + k for k in range(150)] + [26000 + k for k in range(100)] + [33000 + 20 * k for k in range(50)]
        out["dense"] = np.stack([_fill(r, H, W, dense + [0]), _fill(r, H, W, dense[:256] + [7]), _fill(r, H, W, dense[:255] + [7])])
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for (full, small) in COMMUTE_SIZES + [FULL_SIZE]:
        for seed in (1, 2):
            ok, n_full, n_small = commutation_holds(id_image(full[0], full[1], seed), small)
            print("%s -> %s seed %d: %s (%d instances, %d after the zoom)" % (full, small, seed, "equal" if ok else "DIFFERENT", n_full, n_small))
            assert ok
        ok, _, _ = commutation_holds(id_image(full[0], full[1], 3, background=False), small)
        print("%s -> %s without background: %s" % (full, small, "equal" if ok else "DIFFERENT"))
        assert ok
