"""Evaluation driver -- python-3 / MI355X counterpart of reference src/eval.py (a Python-2 file: `print` statements,
`dict.iteritems`), for the part of it that sits on the hot path's output: inference (`test()`), the per-instance
post-processing (`resize_mask`: resample to the original image size, threshold, ignore pixels, minimum size, run-length
encoding -- all on the GPU, rsis_amd/eval_post.py) and the COCO-style prediction records (`create_annotation`,
eval.py:129-142) with the reference's thresholds (-stop_th, -class_th, -mask_th, -min_size; eval.py:299-340).

    python -m rsis_amd.eval --synthetic -model_name <name> -batch_size 32 -maxseqlen 10 [-eval_split test]

writes <models_root>/<model_name>/<model_name>_<eval_split>_predictions.json (list of {image_id, category_id, category_name,
segmentation: COCO RLE, score}) and then, unless --no_run_coco_eval, evaluates them as eval.py:375-398 does (COCOeval 'segm' with
maxDets = [1, -max_dets, 100], useCats = not --ignore_cats, all classes together, then one by one with --all_classes), on the
device (rsis_amd/cocoeval.py): the thresholded masks are bit-packed where they lie, one row per predicted MASK (the C - 1 records
of a mask share it), the ground truth comes from the loader's targets.  The 13 stats are printed in the reference's format and
written to <model_name>_<eval_split>_cocoeval.json.  `-cat_id` is parsed and has no effect, as in the reference (eval.py:381-385
overwrites it).

    python -m rsis_amd.eval -dataset pascal -pascal_dir D -eval_split val -model_name <name> -batch_size 1

evaluates Pascal VOC (eval.py:191-218,280-295): the images come from dataloader/pascal.py in sample order (drop_last=False), every
mask is resampled to its image's ORIGINAL size, the ground truth is <D>/VOCGT_<eval_split>.pkl (rsis_amd.pascal_precompute, or the
reference's own file, python-2 pickle included) and each image's `ignore == 1` record gives the pixels cleared from its predictions.
Nothing is written into the dataset directory (the reference's pascal_<split>.json is an artefact of pycocotools' file interface).

    python -m rsis_amd.eval -dataset cityscapes -cityscapes_dir D ... | -dataset leaves -leaves_dir D ...

(display_cityscapes.sh, display_leaves.sh) read the images through dataloader/cityscapes.py / leaves.py as eval_cityscapes / eval_leaves do,
with the datasets' class names, every mask resampled to its image's original size and no ignore mask; a sample is named as the
reference names it (eval.py:287-291: the Cityscapes path without its extension, the leaves path).  The reference's eval.py has no ground
truth for these two datasets (it stops at an undefined `cocoGT` unless --no_run_coco_eval is given), so the COCO evaluation is skipped for
them, said in one line on stderr; the predictions file is written as for Pascal.

    python -m rsis_amd.eval -dataset coco -coco_dir D -eval_split val -num_classes 81 ...

reads <D>/annotations/instances_<-coco_val_set>.json through dataloader/coco.py (label maps painted on the device), resamples every mask
to its image's original size as for Pascal, without an ignore mask, and scores against the annotation file itself (its records and
`images`; crowd by the evaluator's rule).  The predictions file is a standard COCO results file: the file's integer `image_id`, the
ORIGINAL `category_id` (plus `category_name`); `python -m rsis_amd.cocoeval --gt <annotations> --dt <predictions>` gives the same stats.

    python -m rsis_amd.eval ... --display [--no_display_text] [--display_route]

additionally saves one figure per image (eval.py:342-359), <models_root>/<model_name>/<model_name>_figs_<eval_split>/<name>.png: the
original image (with --synthetic: the de-normalised input) with the RAW mask (before the ignore pixels) of every record kept for display
painted over it in its sequence colour and the class name at the mask's centre -- composited on the device from the byte masks of the
post-processing, rsis_amd/display.py.  The records drawn are those of eval.py:329-338: per timestep the class of maximum confidence when
its score reaches -class_th; for leaves every record of a timestep whose objectness exceeds -stop_th.  Without --display nothing about a
run changes.  A ground-truth FILE of another dataset is evaluated with `python -m rsis_amd.cocoeval`.
Loading the models, opening the reader and loader (or the synthetic loader), the batch loop around `test()` and the `__main__` body are
rsis_amd/eval_common.py, shared with eval_cityscapes.py and eval_leaves.py.  A lone last image is fed to `test()` twice for -dataset
cityscapes and leaves (as eval_leaves.py does) and as it is for pascal, coco and --synthetic.
"""
import json
import os
import sys

import numpy as np
import torch

from .cocoeval import COCOEvalDevice, rle_from_string, run_reference_protocol
from .eval_common import EvalDriver, load_models, run_main  # noqa: F401  (load_models: importable from here as before)
from .eval_post import encode_masks, resize_mask  # noqa: F401  (resize_mask: reference signature, eval.py:96-127)
from .utils.utils import load_plain_pickle


def create_annotation(args, imname, pred_mask, class_id, score, classes, is_valid=True):
    """reference eval.py:129-142: annotation record in the COCO ground-truth format, or None for an invalid mask"""
    if not is_valid:
        return None
    return {"image_id": imname, "category_id": class_id, "category_name": classes[class_id], "segmentation": pred_mask,
            "score": score}


class Evaluate(EvalDriver):
    def __init__(self, args):
        super().__init__(args)
        self.gt_records = self.ignore_rle = None
        self.gt_images = self.category_ids = None                   # -dataset coco: the file's `images`, class index -> category id
        self.display = bool(getattr(args, "display", False))
        self.figures = []                                           # with --display: (path, records drawn, label rectangles) per image
        self.dataset_name = None if getattr(args, "synthetic", False) else args.dataset
        self.no_gt = self.dataset_name in ("cityscapes", "leaves")  # eval.py has no ground truth for them: nothing to evaluate against
        if self.dataset_name is None:
            self.open_synthetic()
            self.class_names = ["<eos>"] + ["class%d" % i for i in range(1, args.num_classes)]
        elif args.dataset == "pascal":
            self._init_pascal()
        elif self.no_gt:
            self._init_files(args.dataset)
        elif args.dataset == "coco":
            self._init_coco()
        else:
            raise Exception("-dataset %s: only --synthetic inputs and -dataset pascal, cityscapes, leaves and coco are wired in this build"
                            % args.dataset)

    def _init_pascal(self):
        """eval.py:191-218 for -dataset pascal"""
        self.open_dataset("pascal")
        self.sample_list = [s.rstrip() for s in self.dataset.get_sample_list()]
        self.gt_records = load_plain_pickle(os.path.join(self.args.pascal_dir, "VOCGT_%s.pkl" % self.split))
        self.ignore_rle = {}                                        # image id -> segmentation of its ignore mask (eval.py:198-209)
        for ann in self.gt_records:
            if ann["ignore"] == 1:
                self.ignore_rle[ann["image_id"]] = ann["segmentation"]

    def _init_coco(self):
        """-dataset coco: the reader of dataloader/coco.py; the ground truth is the annotation file itself, records and `images`"""
        from .cocoeval import load_coco_file
        self.open_dataset("coco")
        self.sample_list = list(self.dataset.image_ids)             # the file's integer image ids
        self.category_ids = list(self.dataset.category_ids)
        self.gt_records, self.gt_images = load_coco_file(self.dataset.ann_file)

    def _init_files(self, name):
        """eval.py:191-218 for -dataset cityscapes / leaves: the reader and loader of eval_cityscapes.py / eval_leaves.py; no ground truth"""
        self.open_dataset(name)
        if name == "cityscapes":
            self.sample_list = [os.path.splitext(f)[0] for f in self.dataset.get_sample_list()]  # eval.py:288
        else:
            self.sample_list = list(self.dataset.get_sample_list())                             # eval.py:291
        if not getattr(self.args, "no_run_coco_eval", False):
            print("-dataset %s has no ground-truth file in eval.py: the COCO evaluation is skipped" % name, file=sys.stderr)

    def _display_image(self, index, x):
        """the (h, w, 3) uint8 image under the figure of sample `index`, on the device: the original file (eval.py:285-293), or with
        --synthetic the input tensor x (3, H, W) de-normalised"""
        from . import display
        if self.dataset is None:
            return display.denormalize(x)
        from PIL import Image
        with Image.open(self.dataset.image_path(index)) as im:
            rgb = np.array(im.convert("RGB"), dtype=np.uint8)
        return torch.as_tensor(rgb).to(x.device)

    def _ignore_mask(self, sample_idx):
        """the (h, w) uint8 ignore mask of one image, decoded from its record (column-major runs, the first one of zeros)"""
        seg = self.ignore_rle[sample_idx]
        h, w = int(seg["size"][0]), int(seg["size"][1])
        counts = rle_from_string(seg["counts"])
        vals = np.arange(len(counts), dtype=np.uint8) & 1
        return np.ascontiguousarray(np.repeat(vals, counts.astype(np.int64)).reshape(w, h).T)

    def _open_evaluator(self):
        """the device evaluator holding the ground truth that comes from a file; None when nothing is evaluated"""
        if getattr(self.args, "no_run_coco_eval", False) or self.no_gt:
            return None
        coco = COCOEvalDevice()
        if self.gt_images is not None:                               # a COCO file: every record, the sizes from its `images`
            coco.add_gt(self.gt_records, images=self.gt_images)
        elif self.gt_records is not None:
            mine = set(self.sample_list)
            coco.add_gt([r for r in self.gt_records if r["image_id"] in mine])
        return coco

    def _image_records(self, sample_idx, segs, areas, raws, scores, stops, h, w):
        """eval.py:303-333 for one image: segs / areas / raws of its T masks (encode_masks), scores (T, C), stops (T, 1) ->
        (predictions: the records of the predictions file, shown: those kept for display, drawn: the same with their mask row,
        rows / cats / recscores: mask row, category id and score of every prediction)"""
        args = self.args
        predictions, shown, drawn, rows, cats, recscores = [], [], [], [], [], []
        classes = np.argmax(scores, axis=-1)

        def record(seg, cls_id, score, is_valid):
            ann = create_annotation(args, sample_idx, _jsonable(seg), cls_id, score, self.class_names, is_valid)
            if ann is not None and self.category_ids is not None:    # a COCO results file: the ORIGINAL id
                ann["category_id"] = self.category_ids[cls_id]
            return ann

        for i in range(scores.shape[0]):
            objectness = float(stops[i][0])
            if objectness < args.stop_th:                          # eval.py:303-304
                continue
            max_class = 1 if args.class_th == 0.0 else int(classes[i])
            is_valid = not (areas[i] < args.min_size * h * w)                                    # eval.py:113-114
            for cls_id in range(1, len(self.class_names)):                                       # eval.py:316-319 (0 = eos)
                score = float(scores[i][cls_id]) * objectness
                ann = record(segs[i], cls_id, score, is_valid)
                if ann is None:
                    continue
                if self.dataset_name == "leaves":                                                # eval.py:329-331
                    if objectness > args.stop_th:
                        shown.append(ann)
                        drawn.append(dict(ann, mask_row=i))
                elif cls_id == max_class and score >= args.class_th:                             # eval.py:333
                    shown.append(record(raws[i], cls_id, score, is_valid))
                    drawn.append(dict(shown[-1], mask_row=i))
                predictions.append(ann)
                rows.append(i)
                cats.append(ann["category_id"])
                recscores.append(score)
        return predictions, shown, drawn, rows, cats, recscores

    def _feed_evaluator(self, sample_idx, targets, h, w, bits, rows, cats, recscores):
        """one image into self.coco: its ground truth from the loader's `targets` (y_mask, y_class, sw_mask of the image) unless a file
        gave it, in the detections' (column-major) element order; its detections as the bit-packed masks that have records"""
        y_mask, y_class, sw_mask = targets
        n_gt = int((sw_mask > 0).sum()) if self.gt_records is None else 0                        # (Pascal, COCO: the records of the file)
        if n_gt:
            gt_m = (y_mask[:n_gt].reshape(n_gt, h, w).transpose(1, 2) > 0.5).to(torch.uint8).reshape(n_gt, h * w)
            self.coco.add_gt_masks(sample_idx, gt_m, [int(c) for c in y_class[:n_gt].cpu()])
        if rows:
            kept = sorted(set(rows))                                 # only the masks that have records go into the pool
            sel = torch.as_tensor(kept, device=bits[0].device)
            pos = {r: j for j, r in enumerate(kept)}
            self.coco.add_dt_masks(sample_idx, None, cats, recscores, rows=[pos[r] for r in rows],
                                   bits=(bits[0][sel], bits[1][sel], bits[2]))

    def _create_json(self):
        """eval.py:254-345: one record per (instance, class) with score = class probability * objectness"""
        args = self.args
        predictions, shown = [], []
        self.coco = self._open_evaluator()
        if self.display:
            from . import display
            figs_dir = display.figures_dir(args.models_root, args.model_name, self.split)       # eval.py:343-344
            os.makedirs(figs_dir, exist_ok=True)
        # eval.py:262; a lone tail image is doubled for -dataset cityscapes / leaves, as eval_leaves.py does; pascal, coco, --synthetic: as it is
        double_lone_tail = self.dataset_name in ("cityscapes", "leaves")
        for first, (x, y_mask, y_class, sw_mask, _sw_class), out_masks, out_scores, stop_probs in self.batches(double_lone_tail):
            scores = out_scores.cpu().numpy()
            stops = stop_probs.cpu().numpy()
            for s in range(out_masks.shape[0]):
                sample_idx = self.sample_list[first + s]
                # eval.py:280-295: the ORIGINAL size and the image's ignore pixels (synthetic images: the input size, none)
                h, w = self.original_size(first + s, (x.size(-2), x.size(-1)))
                ignore = self._ignore_mask(sample_idx) if self.ignore_rle is not None else None
                # all T masks of the image in one launch each: resample + threshold + area, then run-length encoding
                segs, areas, raws, bits, *dev_masks = encode_masks(out_masks[s], h, w, args.mask_th, ignore, want_bits=True,
                                                                   want_masks=self.display)
                new, kept, drawn, rows, cats, recscores = self._image_records(sample_idx, segs, areas, raws, scores[s], stops[s], h, w)
                predictions += new
                shown += kept
                if self.display:                                    # eval.py:342-359: the RAW masks over the original image
                    fig = os.path.join(figs_dir, display.figure_name(sample_idx, self.dataset_name))
                    rects = display.save_figure(fig, self._display_image(first + s, x[s]), dev_masks[0][1], drawn,
                                                no_display_text=args.no_display_text, display_route=args.display_route)
                    self.figures.append((fig, drawn, rects))
                if self.coco is not None:
                    self._feed_evaluator(sample_idx, (y_mask[s], y_class[s], sw_mask[s]), h, w, bits, rows, cats, recscores)
        return predictions, shown

    def run_eval(self):
        predictions, shown = self._create_json()
        out_dir = self.out_path()
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "%s_%s_predictions.json" % (self.args.model_name, self.split))
        with open(path, "w") as f:
            json.dump(predictions, f)
        print("%d prediction records (%d above -class_th for display) from %d images -> %s" %
              (len(predictions), len(shown), len(self.sample_list), path))
        if self.display:
            print("%d figures -> %s" % (len(self.figures), os.path.dirname(self.figures[0][0]) if self.figures else "(none)"))
        if self.coco is not None:                                    # eval.py:375-398
            args = self.args
            cat_ids, img_ids, names = list(range(1, len(self.class_names))), self.sample_list, self.class_names
            if self.category_ids is not None:                       # as `python -m rsis_amd.cocoeval` reads the same two files
                cat_ids = sorted(set(r["category_id"] for r in self.gt_records))
                img_ids = sorted(set(r["image_id"] for r in self.gt_records))
                names = dict(zip(self.category_ids, self.class_names))
            res = run_reference_protocol(self.coco, img_ids, cat_ids, args.max_dets, args.use_cats, args.all_classes, names)
            p = self.coco.params
            res["params"] = {"maxDets": [int(v) for v in p.maxDets], "useCats": int(bool(args.use_cats)), "catIds": cat_ids,
                             "iouThrs": [float(v) for v in p.iouThrs], "recThrs": [float(v) for v in p.recThrs],
                             "areaRng": [[float(v) for v in r] for r in p.areaRng], "areaRngLbl": list(p.areaRngLbl),
                             "images": len(img_ids)}
            epath = os.path.join(out_dir, "%s_%s_cocoeval.json" % (self.args.model_name, self.split))
            with open(epath, "w") as f:
                json.dump(res, f)
            print("COCO segm evaluation -> %s" % epath)
            self.coco_stats = res
        return predictions


def _jsonable(rle):
    return {"size": rle["size"], "counts": rle["counts"].decode("ascii")}


if __name__ == "__main__":
    run_main("rsis_amd.eval", lambda args: Evaluate(args).run_eval())
