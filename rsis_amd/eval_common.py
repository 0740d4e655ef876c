"""What the three evaluation drivers share (eval.py, eval_cityscapes.py, eval_leaves.py; reference src/eval.py:191-262,
eval_cityscapes.py:38-108, eval_leaves.py:36-96): the checkpoint -> eval-mode models (`load_models`), the reader and loader of
-eval_split or the synthetic loader, the batch loop around `test()`, the paths under <models_root>/<model_name>, and the body of
`python -m rsis_amd.<driver>` (`run_main`).  Nothing here knows a dataset: what a driver does with a batch's outputs is its own."""
import os
import sys

import torch

from .args import get_parser
from .modules.model import RSIS, FeatureExtractor
from .synthetic import SyntheticLoader
from .test import test
from .utils.utils import check_parallel, load_checkpoint


def load_models(args):
    """eval.py:229-246 (also eval_cityscapes.py:50-94, eval_leaves.py:45-89): the checkpoint of -model_name under -models_root ->
    eval-mode encoder / decoder on the device, built from the LOADED args; args.num_classes / hidden_size follow the checkpoint.
    Without a checkpoint directory the modules are randomly initialised (synthetic smoke runs), said on stderr."""
    model_dir = os.path.join(args.models_root, args.model_name)
    if os.path.exists(os.path.join(model_dir, "encoder.pt")):
        encoder_dict, decoder_dict, _, _, load_args = load_checkpoint(args.model_name, args.use_gpu, root=args.models_root)
        load_args.use_gpu = args.use_gpu
        if getattr(args, "dtype", None):
            load_args.dtype = args.dtype
        encoder, decoder = FeatureExtractor(load_args), RSIS(load_args)
        encoder_dict, decoder_dict = check_parallel(encoder_dict, decoder_dict)
        encoder.load_state_dict(encoder_dict)
        decoder.load_state_dict(decoder_dict)
        args.num_classes, args.hidden_size = load_args.num_classes, load_args.hidden_size
    else:
        print("no checkpoint at %s: evaluating randomly initialised weights" % model_dir, file=sys.stderr)
        encoder, decoder = FeatureExtractor(args), RSIS(args)
    return encoder.cuda().eval(), decoder.cuda().eval()


class EvalDriver(object):
    """base of the drivers' `Evaluate` classes: after `open_dataset` or `open_synthetic` it has encoder, decoder and loader; a driver
    adds its `sample_list` (how it names the samples) and walks `batches`"""

    def __init__(self, args):
        self.args, self.split, self.T = args, args.eval_split, args.maxseqlen
        self.dataset = None
        if getattr(args, "ignore_regions", False):
            # the drivers share train.py's parser.  The ignore map belongs to the training loss; the measures have their own crowd / group
            # rules.  The readers and the synthetic loader of a driver are opened without it, so every driver sees 5-tuples.
            print("--ignore_regions is a training option: the evaluation drivers do not use it", file=sys.stderr)
            args.ignore_regions = False

    def open_dataset(self, name):
        """eval.py:191-218, the part every dataset shares: the reader of -eval_split with its class names, the models, the loader (file
        order, every sample, the short last batch included)"""
        from .dataloader import eval_loader, open_reader
        self.dataset = open_reader(self.args, self.split, dataset=name)
        self.class_names = self.dataset.get_classes()
        self.encoder, self.decoder = load_models(self.args)
        self.loader = eval_loader(self.args, self.dataset)

    def open_synthetic(self):
        """--synthetic: the models, a few resident synthetic batches and their sample names"""
        args = self.args
        self.encoder, self.decoder = load_models(args)
        self.loader = SyntheticLoader(args, max(1, args.synthetic_batches // 4), args.seed + 7)
        self.sample_list = ["synthetic_%06d" % i for i in range(len(self.loader) * args.batch_size)]

    def batches(self, double_lone_tail):
        """inference over the loader: yields (index of the batch's first sample, the loader's batch tuple, out_masks, out_scores,
        stop_probs), the three outputs with one row per sample of the batch"""
        args, first = self.args, 0
        for batch in self.loader:
            x = batch[0]
            # The reference's test() needs B >= 2 (model.py:169 squeezes the batch axis of a single image away), so a driver whose split
            # may end in a lone image can have it fed twice and the copy's outputs dropped.  test() here takes a batch of one as well;
            # each driver states its choice where it calls this, and keeps it: the other one is another batch shape on the device.
            lone = double_lone_tail and x.size(0) == 1
            outs = test(args, self.encoder, self.decoder, torch.cat([x, x]) if lone else x)
            if lone:
                outs = [t[:1] for t in outs]
            yield (first, batch) + tuple(outs)
            first += x.size(0)

    def original_size(self, index, fallback):
        """(height, width) of sample `index` as its file has it; `fallback` without a dataset (--synthetic)"""
        return self.dataset.raw_size(index) if self.dataset is not None else fallback

    def out_path(self, *parts):
        return os.path.join(self.args.models_root, self.args.model_name, *parts)


def run_main(name, fn):
    """the `__main__` of driver module `name`: the command line, the seed, no GPU -> exit; then fn(args)"""
    args = get_parser().parse_args()
    torch.manual_seed(args.seed)
    if not args.use_gpu or not torch.cuda.is_available():
        raise SystemExit("%s needs the GPU: the HIP library is the only compute path" % name)
    fn(args)
