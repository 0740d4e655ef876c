"""Cityscapes evaluation driver -- python-3 / MI355X counterpart of reference src/eval_cityscapes.py (Python 2): checkpoint ->
`test()` -> per image the result files of the Cityscapes instance-level evaluation script (eval_cityscapes.py:96-174):
`<models_root>/<model_name>/<model_name>_results/<sample>.txt` with one line `<mask png> <class id> <score>` per (timestep, class)
and the mask PNGs (largest connected component of the thresholded mask, resized to the original image) under `<model_name>_masks/`.

    python -m rsis_amd.eval_cityscapes --synthetic -model_name <name> -num_classes 9 -imsize 512 -maxseqlen 20 -batch_size 8 [-dtype bf16]

    python -m rsis_amd.eval_cityscapes -cityscapes_dir D -eval_split val -model_name <name> -num_classes 9 -imsize 256 -maxseqlen 20

Without `--synthetic` the images of `-eval_split` come from dataloader/cityscapes.py in sorted file order (shuffle=False,
drop_last=False, no augmentation), a sample is named after its file (`<city>_<seq>_<frame>_leftImg8bit`, eval_cityscapes.py:114-120),
the masks are resized to the size in the PNG header, and the ground truth scored against is the raw array of each image's
`*_gtFine_instanceIds.png`: nothing is written into the dataset directory and no `_gt` copy is made.
With `--synthetic`: square images of `-imsize` whose "original" size is taken as twice that, which exercises the same resize path.
Everything after `test()` is the reference's procedure, through
`rsis_amd.eval_post.write_cityscapes_results`.  Deviations from the reference script: an empty mask is written as an
all-zero PNG (the reference reuses a stale `max_label` from the previous mask); scores are formatted from float64 (the reference
prints numpy float32 `str`), i.e. more digits of the same number.

The reference stops here and leaves the numbers to the benchmark's evaluation script.  This driver goes on: unless `--no_run_coco_eval`
is given (the flag the reference's scripts pass to skip scoring; same meaning here) the masks just written are scored against the
ground truth with `rsis_amd.cityscapes_eval` (AP, AP50% per class; pixel counting on the device), the table is printed and
`<models_root>/<model_name>/<model_name>_cityscapes_eval.json` is written.  With `--synthetic` the ground truth is stored the way the
benchmark stores it, `<model_name>_gt/<sample>_gtFine_instanceIds.png` (16-bit, at the "original" size by pixel replication):
instance k of class c >= 1 of the loader's targets has the value CITYSCAPES_CLASS_IDS[c - 1] * 1000 + k, the earlier instance keeps a
contested pixel, the background is 7 (road: neither void nor an instance; 0 would make every false positive "ignored").
`python -m rsis_amd.cityscapes_eval --results <..._results> --gt <..._gt>` gives the same JSON from the files.
`--display` is parsed and ignored here, as in the reference's eval_cityscapes.py (it stores the flag and never reads it); the figures of
`--display` (display_cityscapes.sh) come from `python -m rsis_amd.eval -dataset cityscapes ... --display`.
"""
import os
import sys

import numpy as np
import torch

from .args import get_parser
from .eval import load_models
from .eval_post import CITYSCAPES_CLASS_IDS, write_cityscapes_results
from .synthetic import SyntheticLoader
from .test import test


BACKGROUND_ID = 7


def synthetic_instance_ids(y_mask, y_class, height, width, scale=2):
    """(T, height * width) 0 / 1 masks and (T,) classes of one image's targets -> (scale * height, scale * width) uint16 instance-id
    image (module docstring)"""
    m = np.asarray(y_mask.detach().cpu()).reshape(-1, height, width) > 0.5
    c = np.asarray(y_class.detach().cpu()).reshape(-1)
    gt = np.full((height, width), BACKGROUND_ID, np.uint16)
    free = np.ones((height, width), bool)
    for k in range(m.shape[0]):
        if c[k] < 1:
            continue
        cid = CITYSCAPES_CLASS_IDS[c[k] - 1] if c[k] - 1 < len(CITYSCAPES_CLASS_IDS) else int(c[k])
        gt[m[k] & free] = cid * 1000 + k
        free &= ~m[k]
    return np.repeat(np.repeat(gt, scale, 0), scale, 1)


class Evaluate(object):
    def __init__(self, args):
        self.args, self.split, self.T = args, args.eval_split, args.maxseqlen
        self.dataset = None
        if not getattr(args, "synthetic", False):
            self._init_files()
            return
        self.encoder, self.decoder = load_models(args)
        self.loader = SyntheticLoader(args, max(1, args.synthetic_batches // 4), args.seed + 7)
        self.sample_list = ["synthetic_%06d" % i for i in range(len(self.loader) * args.batch_size)]

    def _init_files(self):
        """eval_cityscapes.py:38-51: the images of -eval_split through the reader, in file order"""
        from .dataloader import eval_loader, open_reader
        args = self.args
        self.dataset = open_reader(args, self.split, dataset="cityscapes")
        self.sample_list = [os.path.basename(f).split(".")[0] for f in self.dataset.get_sample_list()]   # :114-120
        self.encoder, self.decoder = load_models(args)
        self.loader = eval_loader(args, self.dataset)

    def _create_figures_files(self):
        """create_figures on the files of the dataset: original sizes from the PNG headers, ground truth = the raw instanceIds arrays"""
        from . import cityscapes_eval
        args = self.args
        results_dir = os.path.join(args.models_root, args.model_name, args.model_name + "_results")     # eval_cityscapes.py:99-104
        masks_dir = args.model_name + "_masks"
        os.makedirs(os.path.join(results_dir, masks_dir), exist_ok=True)
        self.results_dir, self.gt_dir = results_dir, None
        do_score = not getattr(args, "no_run_coco_eval", False)
        self.records = []
        print("Creating annotations for cityscapes validation...")
        acc, n_lines = 0, 0
        for x, _y_mask, _y_class, _sw_mask, _sw_class in self.loader:
            out_masks, out_scores, stop_probs = test(args, self.encoder, self.decoder, x)               # :108
            Hm, Wm = x.size(-2), x.size(-1)
            gts, mask_sets, rows, labels, scores = [], [], [], [], []
            for s in range(out_masks.shape[0]):
                sample, masks = self.sample_list[s + acc], []
                h, w = self.dataset.raw_size(s + acc)                                                    # :115-118
                lines = write_cityscapes_results(args, sample, out_masks[s].view(self.T, Hm, Wm), out_scores[s],
                                                 stop_probs[s], h, w, results_dir, masks_dir, collect=masks)
                n_lines += len(lines)
                if do_score:
                    gts.append(cityscapes_eval.read_gt_png(self.dataset.ins_files[s + acc]))
                    mask_sets.append(masks)
                    rows.append([q // (len(lines) // len(masks)) for q in range(len(lines))])
                    labels.append([int(l.split()[1]) for l in lines])
                    scores.append([float(l.split()[2]) for l in lines])
            if do_score:
                self.records += cityscapes_eval.score_image_sets(gts, mask_sets, rows, labels, scores)
            acc += out_masks.shape[0]
        print("%d result lines for %d images -> %s" % (n_lines, acc, results_dir))
        return n_lines

    def create_figures(self):
        if self.dataset is not None:
            return self._create_figures_files()
        args = self.args
        results_dir = os.path.join(args.models_root, args.model_name, args.model_name + "_results")     # eval_cityscapes.py:99-104
        masks_dir = args.model_name + "_masks"
        os.makedirs(os.path.join(results_dir, masks_dir), exist_ok=True)
        self.results_dir = results_dir
        self.gt_dir = os.path.join(args.models_root, args.model_name, args.model_name + "_gt")
        os.makedirs(self.gt_dir, exist_ok=True)
        do_score = not getattr(args, "no_run_coco_eval", False)
        self.records = []
        print("Creating annotations for cityscapes validation...")
        from PIL import Image
        from . import cityscapes_eval
        acc, n_lines = 0, 0
        for x, y_mask, y_class, _sw_mask, _sw_class in self.loader:
            out_masks, out_scores, stop_probs = test(args, self.encoder, self.decoder, x)               # :108
            Hm, Wm = x.size(-2), x.size(-1)
            gts, mask_sets, rows, labels, scores = [], [], [], [], []
            for s in range(out_masks.shape[0]):
                sample, masks = self.sample_list[s + acc], []
                gt = synthetic_instance_ids(y_mask[s], y_class[s], Hm, Wm)
                Image.fromarray(gt).save(os.path.join(self.gt_dir, sample + cityscapes_eval.GT_SUFFIX))
                lines = write_cityscapes_results(args, sample, out_masks[s].view(self.T, Hm, Wm), out_scores[s],
                                                 stop_probs[s], 2 * Hm, 2 * Wm, results_dir, masks_dir, collect=masks)
                n_lines += len(lines)
                gts.append(gt)
                mask_sets.append(masks)
                rows.append([q // (len(lines) // len(masks)) for q in range(len(lines))])
                labels.append([int(l.split()[1]) for l in lines])
                scores.append([float(l.split()[2]) for l in lines])
            if do_score:                                           # the arrays that were just saved: nothing is read back
                self.records += cityscapes_eval.score_image_sets(gts, mask_sets, rows, labels, scores)
            acc += out_masks.shape[0]
        print("%d result lines for %d images -> %s" % (n_lines, acc, results_dir))
        return n_lines

    def score(self):
        """AP / AP50% of what `create_figures` wrote: prints the table, writes <model_name>_cityscapes_eval.json next to the results folder
        and returns the result dict; None under --no_run_coco_eval"""
        from . import cityscapes_eval
        args = self.args
        if getattr(args, "no_run_coco_eval", False):
            print("--no_run_coco_eval: the result files are not scored")
            return None
        aps = cityscapes_eval.evaluate_matches(self.records)
        res = {"aps": aps, "averages": cityscapes_eval.compute_averages(aps), "images": len(self.records)}
        sys.stdout.write(cityscapes_eval.summary(res["averages"]))
        name = os.path.join(args.models_root, args.model_name, args.model_name + "_cityscapes_eval.json")
        print("%d images -> %s" % (res["images"], cityscapes_eval.write_result_json(name, res)))
        return res


if __name__ == "__main__":
    a = get_parser().parse_args()
    torch.manual_seed(a.seed)
    if not a.use_gpu or not torch.cuda.is_available():
        raise SystemExit("rsis_amd.eval_cityscapes needs the GPU: the HIP library is the only compute path")
    ev = Evaluate(a)
    ev.create_figures()
    ev.score()
    sys.exit(0)
