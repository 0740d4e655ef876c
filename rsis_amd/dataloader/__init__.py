"""The data layer (reference src/dataloader/), SURVEY.md section 8(f) row N3:
  targets   : an instance-id map + a class map -> what `runIter` consumes (dataset.py:86-146);
  augment   : the affine augmentation;
  reader    : the base class of the dataset readers -- constructor state, decode cache, resize, flip / crop draws, `host_item` -- and
              the few hooks a reader provides to the loader;
  leaves, pascal, cityscapes, coco : the four readers (CVPPP A1 of BASELINE configs[0]; Pascal VOC, whose ProcMasks / VOCGT_<split>.pkl
              come from `python -m rsis_amd.pascal_precompute`; Cityscapes, raw ids on the host and both maps on the device; a standard
              COCO instances file, polygons staged on the host and both maps painted on the device);
  loader    : DeviceLoader, the pinned staging and device batch path of every reader.
`open_reader` and `eval_loader` are how train.py and the evaluation drivers open them.  Importing this package loads neither the readers
nor the HIP library."""
import importlib

from .targets import sequence_from_masks, targets_from_maps  # noqa: F401

READERS = {"leaves": ("leaves", "LeavesDataset"), "pascal": ("pascal", "PascalVOC"), "cityscapes": ("cityscapes", "CityScapes"),
           "coco": ("coco", "COCO")}                      # -dataset -> (module, class)


def open_reader(args, split, augment=False, dataset=None):
    """the reader of `dataset` (default: -dataset) on `split`, with -resize and -imsize"""
    module, name = READERS[dataset or args.dataset]
    cls = getattr(importlib.import_module("." + module, __name__), name)
    return cls(args, split=split, augment=augment, resize=args.resize, imsize=args.imsize)


def eval_loader(args, reader):
    """the loader of the evaluation drivers: file order, every sample, the short last batch included"""
    from .loader import DeviceLoader
    return DeviceLoader(reader, args.batch_size, shuffle=False, num_workers=args.num_workers, seed=args.seed, drop_last=False)
