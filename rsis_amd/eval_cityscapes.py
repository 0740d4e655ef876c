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
Opening the reader or the synthetic loader and the models, the batch loop around `test()` and the `__main__` body are
rsis_amd/eval_common.py, shared with eval.py and eval_leaves.py; the two modes differ in `_ground_truth` alone.
"""
import os
import sys

import numpy as np

from .eval_common import EvalDriver, run_main
from .eval_post import CITYSCAPES_CLASS_IDS, cityscapes_result_columns, write_cityscapes_results


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


class Evaluate(EvalDriver):
    def __init__(self, args):
        super().__init__(args)
        if getattr(args, "synthetic", False):
            self.open_synthetic()
        else:                                  # eval_cityscapes.py:38-51: the images of -eval_split through the reader, in file order
            self.open_dataset("cityscapes")
            self.sample_list = [os.path.basename(f).split(".")[0] for f in self.dataset.get_sample_list()]   # :114-120

    def _ground_truth(self, index, sample, y_mask, y_class, Hm, Wm, do_score):
        """what one image is scored against and resized to: (instance-id array or None, height, width).  Files: the raw instanceIds array,
        read only when it is scored, and the size in the PNG header.  --synthetic: the array made of the loader's targets, saved as the
        benchmark stores it whether scored or not (nothing is read back), and twice the input size."""
        from . import cityscapes_eval
        if self.dataset is not None:
            gt = cityscapes_eval.read_gt_png(self.dataset.ins_files[index]) if do_score else None
        else:
            from PIL import Image
            gt = synthetic_instance_ids(y_mask, y_class, Hm, Wm)
            Image.fromarray(gt).save(os.path.join(self.gt_dir, sample + cityscapes_eval.GT_SUFFIX))
        return (gt,) + tuple(self.original_size(index, (2 * Hm, 2 * Wm)))                              # :115-118

    def create_figures(self):
        from . import cityscapes_eval
        args = self.args
        results_dir = self.out_path(args.model_name + "_results")                                       # eval_cityscapes.py:99-104
        masks_dir = args.model_name + "_masks"
        os.makedirs(os.path.join(results_dir, masks_dir), exist_ok=True)
        self.results_dir, self.gt_dir = results_dir, None
        if self.dataset is None:
            self.gt_dir = self.out_path(args.model_name + "_gt")
            os.makedirs(self.gt_dir, exist_ok=True)
        do_score = not getattr(args, "no_run_coco_eval", False)
        self.records = []
        print("Creating annotations for cityscapes validation...")
        n_images = n_lines = 0
        for first, (x, y_mask, y_class, *_sw), out_masks, out_scores, stop_probs in self.batches(False):   # :108; a lone tail image as it is
            Hm, Wm = x.size(-2), x.size(-1)
            gts, mask_sets, rows, labels, scores = [], [], [], [], []
            for s in range(out_masks.shape[0]):
                sample, masks = self.sample_list[first + s], []
                gt, h, w = self._ground_truth(first + s, sample, y_mask[s], y_class[s], Hm, Wm, do_score)
                lines = write_cityscapes_results(args, sample, out_masks[s].view(self.T, Hm, Wm), out_scores[s],
                                                 stop_probs[s], h, w, results_dir, masks_dir, collect=masks)
                n_lines += len(lines)
                if do_score:
                    gts.append(gt)
                    mask_sets.append(masks)
                    for column, values in zip((rows, labels, scores), cityscapes_result_columns(lines, len(masks))):
                        column.append(values)
            if do_score:
                self.records += cityscapes_eval.score_image_sets(gts, mask_sets, rows, labels, scores)
            n_images += out_masks.shape[0]
        print("%d result lines for %d images -> %s" % (n_lines, n_images, results_dir))
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
        name = self.out_path(args.model_name + "_cityscapes_eval.json")
        print("%d images -> %s" % (res["images"], cityscapes_eval.write_result_json(name, res)))
        return res


def _main(args):
    ev = Evaluate(args)
    ev.create_figures()
    ev.score()


if __name__ == "__main__":
    run_main("rsis_amd.eval_cityscapes", _main)
