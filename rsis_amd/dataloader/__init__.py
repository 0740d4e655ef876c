"""Target-tensor construction of the reference's data layer (reference src/dataloader/dataset.py:86-146), SURVEY.md section
8(f) row N3: the step that turns an instance-id map + a class map into what `runIter` consumes (targets), the affine augmentation
(augment), and the CVPPP A1 leaves reader + device batch loader of BASELINE configs[0] (leaves), and the Pascal VOC reader on the same loader
(pascal; its ProcMasks / VOCGT_<split>.pkl come from `python -m rsis_amd.pascal_precompute`), and the Cityscapes reader on the same
loader (cityscapes: the host resamples the raw `*_gtFine_instanceIds.png` values, the device derives class map and compact instance
map from them -- rsis_instance_maps), and the COCO reader on the same loader (coco: a standard instances file; the host stages the
batch's polygons and index tables, the device rasterises them and paints both maps -- rsis_poly_to_bits, rsis_paint_instance_maps)."""
from .targets import sequence_from_masks, targets_from_maps  # noqa: F401
