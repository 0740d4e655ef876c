"""CVPPP leaf segmentation challenge measures on the device -- what the reference obtained from the challenge's Matlab scripts
(src/CVPPP/LSC_Evaluation.m and its helpers) for the label images `rsis_amd.eval_leaves` writes.  No Matlab, no Octave: the measures
are restated from their definitions and computed by two grouped launches of rsis_amd/csrc/labeleval.hip.

    python -m rsis_amd.cvppp_eval --results DIR --gt DIR [--user NAME] [--out DIR]

For one pair of equally sized 8-bit label images `in` (result) and `gt`, with n_i = pixels of `in` with value i, m_j = pixels of `gt`
with value j, o_ij = pixels with both, lo_a / hi_a the smallest / largest value present in image a:

  Dice(i, j)        = 2 o_ij / (n_i + m_j), one float64 division of two integers; 0 / 0 counts as 0 (it never wins a maximum)
  BestDice(in, gt)  = (sum over EVERY integer i of lo_in .. hi_in, ascending, of max(0, max_{j in lo_gt .. hi_gt} Dice(i, j)))
                      / (hi_in - lo_in + 1): the background value takes part like any label, a value of the range that does not occur
                      adds 0 and still counts in the divisor (the challenge's script assumes consecutive labels; `leaves_label_image`
                      can leave gaps)
  SymmetricBestDice = min(BestDice(in, gt), BestDice(gt, in))
  FgBgDice          = 2 |F_in and F_gt| / (|F_in| + |F_gt|), F_a = {a > lo_a}; NaN when both images are constant (kept as NaN)
  DiffFGLabels      = (hi_in - lo_in) - (hi_gt - lo_gt), AbsDiffFGLabels its absolute value

A score row is SCORE_COLUMNS: these four and the two one-sided BestDice values.  Every count is an integer and every score a float64
expression of integers in a fixed order, so the device results are the same bits as a plain numpy statement of the definitions.

Deviations, deliberate:
  * a result image of another size than its ground truth is brought to that size by nearest-neighbour sampling with the pixel-centre
    rule src = min(floor((d + 0.5) * n_in / n_out), n_in - 1) per axis.  This is OUR rule: whether Matlab's imresize(..., 'nearest')
    picks the same pixels was not checked, so a warning is issued whenever it is taken (`eval_leaves` writes at the original size and
    never takes it);
  * label images are 8-bit greyscale or palette PNGs, read as their index values; RGB(A), 16-bit and bilevel files are refused;
  * the summary rows use numpy's mean / std (n - 1) / median / max / min, which propagate a NaN; it is written as `NaN`.
"""
import argparse
import glob
import os
import re
import sys
import warnings

import numpy as np
import torch

from ._lib import _device, check, lib, ptr, stream

SCORE_COLUMNS = ("SymmetricBestDice", "FgBgDice", "AbsDiffFGLabels", "DiffFGLabels", "BestDice_in_gt", "BestDice_gt_in")
TABLE = 256 * 256            # uint32 counts of one pair in the dense global table: counts[i * 256 + j]
SUMMARY_ROWS = ("mean", "std", "median", "max", "min")


# ------------------------------------------------------------------ the two launches ------------------------------------------------------------------
def nearest_index(n_in, n_out):
    """source index of every destination index of one axis: min(floor((d + 0.5) * n_in / n_out), n_in - 1), in integers"""
    d = np.arange(int(n_out), dtype=np.int64)
    return np.minimum(((2 * d + 1) * int(n_in)) // (2 * int(n_out)), int(n_in) - 1)


def resize_nearest(img, height, width):
    """(h, w) tensor -> (height, width) by the pixel-centre nearest rule of the module docstring"""
    iy = torch.from_numpy(nearest_index(img.shape[0], height)).to(img.device)
    ix = torch.from_numpy(nearest_index(img.shape[1], width)).to(img.device)
    return img.index_select(0, iy).index_select(1, ix)


def job_table(npix, align=16, blocks_of=None):
    """The pool layout and the job table of a call: for pair p the images lie at in_off / gt_off of one byte pool (each start rounded up
    to `align` bytes; align = 1 packs them back to back, which the kernel takes as well), its table at p * TABLE.  Returns
    (jobs (N, 8) int64 = {in_off, gt_off, npix, table_off, block_begin, 0, 0, 0}, pool length, total blocks)."""
    if blocks_of is None:
        blocks_of = lib().rsis_label_contingency_blocks
    jobs = np.zeros((len(npix), 8), np.int64)
    off = blk = 0
    up = lambda v: -(-v // align) * align
    for p, n in enumerate(npix):
        n = int(n)
        if n < 1 or n >= 1 << 32:
            raise ValueError("pair %d: %d pixels (1 .. 2^32 - 1 are supported)" % (p, n))
        in_off = up(off)
        gt_off = up(in_off + n)
        off = gt_off + n
        jobs[p, :5] = (in_off, gt_off, n, p * TABLE, blk)
        blk += int(blocks_of(n))
    return jobs, off, blk


def _as_label_tensor(x, what):
    t = torch.as_tensor(x)
    if t.dtype != torch.uint8 or t.dim() != 2 or t.numel() < 1:
        raise ValueError("%s: label images are non-empty 2-d uint8 tensors (got %s %s)" % (what, t.dtype, tuple(t.shape)))
    return t


def _pool(in_images, gt_images, align, device):
    """-> (pool uint8 device tensor, jobs device tensor, N, total blocks); ONE host -> device copy of the pool when the images are on the host"""
    if len(in_images) != len(gt_images):
        raise ValueError("%d result images for %d ground-truth images" % (len(in_images), len(gt_images)))
    pairs = []
    for k, (a, g) in enumerate(zip(in_images, gt_images)):
        a, g = _as_label_tensor(a, "in[%d]" % k), _as_label_tensor(g, "gt[%d]" % k)
        if a.shape != g.shape:
            warnings.warn("pair %d: result %dx%d resampled to the ground truth's %dx%d by the pixel-centre nearest rule (our rule, not "
                          "checked against Matlab's imresize)" % (k, a.shape[0], a.shape[1], g.shape[0], g.shape[1]))
            a = resize_nearest(a, g.shape[0], g.shape[1])
        pairs.append((a, g))
    jobs, length, blocks = job_table([g.numel() for _a, g in pairs], align)
    on_host = all(not t.is_cuda for pr in pairs for t in pr)
    pool = torch.zeros((length + 15) // 16 * 16, dtype=torch.uint8, device="cpu" if on_host else device)
    for (a, g), J in zip(pairs, jobs):
        pool[J[0]:J[0] + J[2]] = a.reshape(-1).to(pool.device)
        pool[J[1]:J[1] + J[2]] = g.reshape(-1).to(pool.device)
    return pool.to(device), torch.from_numpy(jobs).to(device), len(pairs), blocks


def _launch_contingency(pool, jobs, n, blocks):
    counts = torch.empty((n * TABLE,), dtype=torch.int32, device=pool.device)
    check(lib().rsis_label_contingency_batch(ptr(pool), pool.numel(), ptr(jobs), n, blocks, ptr(counts), counts.numel(), stream()),
          "rsis_label_contingency_batch")
    return counts


def _launch_scores(counts, jobs, n):
    scores = torch.empty((n, 6), dtype=torch.float64, device=counts.device)
    check(lib().rsis_label_scores_batch(ptr(counts), counts.numel(), ptr(jobs), n, ptr(scores), stream()), "rsis_label_scores_batch")
    return scores


def contingency(in_images, gt_images, device="cuda", align=16):
    """lists of N uint8 (h, w) tensors / arrays, host or device, any sizes -> (N, 256, 256) int64 device tensor, [p, i, j] = number of
    pixels of pair p with in == i and gt == j (one grouped launch)"""
    device = _device(device, "rsis_amd.cvppp_eval")
    if len(gt_images) == 0:
        return torch.zeros((0, 256, 256), dtype=torch.int64, device=device)
    pool, jobs, n, blocks = _pool(in_images, gt_images, align, device)
    counts = _launch_contingency(pool, jobs, n, blocks)
    return (counts.to(torch.int64) & 0xFFFFFFFF).view(n, 256, 256)


def score_pairs(in_images, gt_images, device="cuda", align=16):
    """lists of N uint8 (h, w) tensors / arrays -> (N, 6) float64 host tensor, columns SCORE_COLUMNS: the contingency launch, the scores
    launch, one device -> host copy"""
    device = _device(device, "rsis_amd.cvppp_eval")
    if len(gt_images) == 0:
        return torch.zeros((0, 6), dtype=torch.float64)
    pool, jobs, n, blocks = _pool(in_images, gt_images, align, device)
    return _launch_scores(_launch_contingency(pool, jobs, n, blocks), jobs, n).cpu()


# ------------------------------------------------------------------ files and tables ------------------------------------------------------------------
def plant_number(path):
    """the last number in the file name (plant017_label.png -> 17)"""
    found = re.findall(r"\d+", os.path.basename(path))
    if not found:
        raise ValueError("%s: no plant number in the file name" % path)
    return int(found[-1])


def read_label_png(path):
    """8-bit greyscale or palette PNG -> (h, w) uint8 array of its (index) values; anything else is refused"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "P"):
            raise ValueError("%s: mode %r is not a label image this evaluation reads: 8-bit greyscale ('L') or palette ('P') only -- RGB(A), "
                             "16-bit and bilevel label images are refused" % (path, im.mode))
        a = np.array(im)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("%s: decoded as %s %s, not as 8-bit labels" % (path, a.dtype, a.shape))
    return a


def evaluate_files(result_files, gt_files, score_fn=None):
    """One row per ground-truth file, in ascending plant number; the result file with the same plant number is its partner, a ground
    truth without one is scored against an all-zero image; result files without a ground truth are ignored.  Returns (numbers list,
    (N, 6) float64 tensor)."""
    score_fn = score_fn or score_pairs
    res = {}
    for f in result_files:
        k = plant_number(f)
        if k in res:
            raise ValueError("two result files for plant %d: %s and %s" % (k, res[k], f))
        res[k] = f
    gts = sorted((plant_number(f), f) for f in gt_files)
    numbers = [k for k, _f in gts]
    if len(set(numbers)) != len(numbers):
        raise ValueError("two ground-truth files share a plant number")
    ins, gt_imgs = [], []
    for k, f in gts:
        g = read_label_png(f)
        if k in res:
            a = read_label_png(res[k])
        else:
            print("plant %d: no result image, scored against an all-zero image" % k)
            a = np.zeros_like(g)
        ins.append(torch.from_numpy(a))
        gt_imgs.append(torch.from_numpy(g))
    scores = torch.as_tensor(score_fn(ins, gt_imgs), dtype=torch.float64).reshape(len(gts), 6)
    return numbers, scores


def evaluate_dirs(result_dir, gt_dir, experiment="A1", score_fn=None):
    """`*_label.png` of gt_dir (or of gt_dir/<experiment> when that folder exists) against `*_label.png` of result_dir (likewise)"""
    pick = lambda d: os.path.join(d, experiment) if os.path.isdir(os.path.join(d, experiment)) else d
    gt_files = sorted(glob.glob(os.path.join(pick(gt_dir), "*_label.png")))
    if not gt_files:
        raise ValueError("no *_label.png ground truth under %s" % pick(gt_dir))
    return evaluate_files(sorted(glob.glob(os.path.join(pick(result_dir), "*_label.png"))), gt_files, score_fn)


def summary(scores):
    """(N, >= 4) scores -> (5, 4) float64 array: SUMMARY_ROWS of the four table columns (std: sample, n - 1)"""
    s = np.asarray(scores, dtype=np.float64).reshape(-1, np.shape(scores)[-1])[:, :4]
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if s.shape[0] == 0:
            return np.full((5, 4), np.nan)
        return np.stack([s.mean(0), s.std(0, ddof=1) if s.shape[0] > 1 else np.full((4,), np.nan), np.median(s, 0), s.max(0), s.min(0)])


def _f(v):
    return "NaN" if np.isnan(v) else "%f" % v


def result_table_text(numbers, scores, experiment="A1"):
    s = np.asarray(scores, dtype=np.float64).reshape(len(numbers), -1)
    lines = ["Results for images: %s" % experiment, "", "number, SymmetricBestDice, FGBGDice, AbsDiffFGLabels, DiffFGLabels"]
    for k, r in zip(numbers, s):
        lines.append("%d, %s, %s, %d, %d" % (k, _f(r[0]), _f(r[1]), int(r[2]), int(r[3])))
    lines.append("")
    for name, r in zip(SUMMARY_ROWS, summary(s)):
        lines.append("%s, %s" % (name, ", ".join(_f(v) for v in r)))
    return "\n".join(lines) + "\n"


def write_result_table(path, user, numbers, scores, experiment="A1"):
    """<path>/<user>_<experiment>_results.csv in the layout of the challenge's per-experiment table; returns the file name"""
    os.makedirs(path, exist_ok=True)
    name = os.path.join(path, "%s_%s_results.csv" % (user, experiment))
    with open(name, "w") as f:
        f.write(result_table_text(numbers, scores, experiment))
    return name


def print_summary(scores, out=None):
    out = out or sys.stdout
    out.write("        SymmetricBestDice, FGBGDice, AbsDiffFGLabels, DiffFGLabels\n")
    for name, r in zip(SUMMARY_ROWS, summary(scores)):
        out.write("%s, %s\n" % (name, ", ".join(_f(v) for v in r)))


def get_cli_parser():
    p = argparse.ArgumentParser(prog="python -m rsis_amd.cvppp_eval", description="CVPPP A1 measures of a folder of label images")
    p.add_argument("--results", required=True, help="folder of the result plantNNN_label.png files (or its parent holding A1/)")
    p.add_argument("--gt", required=True, help="folder of the ground-truth plantNNN_label.png files")
    p.add_argument("--user", default="rsis", help="name in front of _A1_results.csv")
    p.add_argument("--out", default=None, help="folder of the CSV (default: --results)")
    return p


def main(argv=None):
    a = get_cli_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rsis_amd.cvppp_eval needs the GPU: the HIP library is the only compute path")
    numbers, scores = evaluate_dirs(a.results, a.gt)
    print_summary(scores)
    name = write_result_table(a.out or a.results, a.user, numbers, scores)
    print("%d images -> %s" % (len(numbers), name))
    return numbers, scores


if __name__ == "__main__":
    main()
