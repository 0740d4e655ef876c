"""The device batch loader of every reader (reader.py: leaves, pascal, cityscapes, coco) -- DataLoader(dataset, batch_size,
shuffle=True, drop_last=True) of the reference's train.py:46-49, yielding what utils.batch_to_var returns, on the device.

Split of the work:
  host   : the reader's `host_item` per sample (decode, resize, flip, crop: reader.py) into PINNED staging buffers, by a small thread
           pool one batch ahead; the reader's `stage_batch` per batch (COCO: the polygons and index tables as one int64 table); the draw of
           the affine matrices (python `random`, same draw order as the reference);
  device : uint8 -> float, ImageNet normalisation (train.py:34-37), the reader's `maps_to_warp`, the affine warp of image and maps
           (rsis_affine_nearest, bit-equal to the reference's th_affine2d(mode='nearest')), the reader's `label_maps`, and the target
           tensors runIter reads (targets_from_maps == sequence_from_masks + batch_to_var).
The loader asks its dataset only what reader.Reader states: `num_maps`, `same_size`, `crop`, `max_seq_len`, `augmentation_transform`,
`host_item`, the four hooks, and `_cache` (to keep cache hits off the pool)."""
import random
import threading
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .augment import affine_nearest
from .targets import targets_from_maps

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def shard_batches(order, batch_size, rank=0, world=1, drop_last=True):
    """Per-rank index lists of one epoch: the (already shuffled, identical on every rank) sample order is cut into GLOBAL batches of
    batch_size * world (the tail that does not fill one is dropped: drop_last=True, train.py:46-49) and rank r takes elements
    r, r + world, ... of each -- the ranks' shards of a step are disjoint and together are the reference's global batch."""
    gb = int(batch_size) * int(world)
    out = [order[i * gb:(i + 1) * gb][rank::world] for i in range(len(order) // gb)]
    if not drop_last and len(order) % gb and int(world) == 1:       # evaluation (eval*.py: drop_last=False): the short last batch
        out.append(order[len(order) // gb * gb:])
    return out


class PinnedSet(object):
    """pinned staging tensors, reused: `torch.empty(...).pin_memory()` per batch is a hipHostMalloc + first-touch page faults -- 1.9 of
    the 2.15 ms a batch of two CACHED samples took to stage (tools/exp/stage_bench.py), more than the GPU needs for a tenth of its
    step.  Filled through the numpy views (a torch CPU copy_ of 200 KB costs ~1 ms of thread-pool wake-up); refilled only after the
    host-to-device copies that last read it have completed (`event`)."""

    def __init__(self, shapes, dtypes):
        self.tensors = [torch.empty(tuple(s), dtype=d).pin_memory() for s, d in zip(shapes, dtypes)]
        self.views = [t.numpy() for t in self.tensors]
        self.event = None

    def wait(self):
        """wait for the event, then clear it: the set may be written again"""
        if self.event is not None:
            self.event.synchronize()
            self.event = None

    def record(self, stream):
        self.event = torch.cuda.Event()
        self.event.record(stream)


# one staged batch: the pinned image (B, 3, H, W) uint8, the pinned int32 maps, the pinned int64 table with its layout (or None, None),
# the affine matrices (or None), and the pinned sets the copies read
Staged = namedtuple("Staged", "image maps table layout mats pins")


class DeviceLoader(object):
    """yields DEVICE batches (x, y_mask, y_class, sw_mask, sw_class), and a sixth tensor, the (B, N) uint8 ignore map, when the reader's
    `ignore_map` hook answers (--ignore_regions on coco / cityscapes).  The next batch is decoded into pinned memory by `num_workers`
    threads and copied on a side stream while the current one trains.

    One process per GPU (rank / world): `batch_size` is the PER-RANK batch; every rank shuffles the whole dataset with the SAME
    seed and takes samples r, r + world, ... of each global batch of batch_size * world, so that an epoch is
    len(dataset) // (batch_size * world) steps of the reference's global batch (train.py:46-49 under nn.DataParallel) and no
    sample is seen twice in a step; only the per-sample augmentation draws are rank-specific."""

    def __init__(self, dataset, batch_size, shuffle=True, num_workers=4, seed=0, device="cuda", rank=0, world=1, drop_last=True):
        self.drop_last = bool(drop_last)
        if dataset.crop is False and batch_size != 1 and not dataset.same_size:
            raise ValueError("un-cropped samples have different sizes: batch_size must be 1")
        self.ds, self.bs, self.shuffle, self.device = dataset, int(batch_size), shuffle, device
        self.rank, self.world = int(rank), int(world)
        self.order_rng = random.Random(seed)                                # the same on every rank
        self.rng = random.Random(seed * 1000003 + 17 * self.rank + 1)       # per-sample draws (crop / flip / warp)
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(num_workers)))
        self.copy_stream = torch.cuda.Stream() if torch.cuda.is_available() else None
        self.mean = torch.tensor(MEAN, device=device).view(1, 3, 1, 1)
        self.std = torch.tensor(STD, device=device).view(1, 3, 1, 1)
        self._lock = threading.Lock()
        self._pins = {}

    def __len__(self):
        n, gb = len(self.ds), self.bs * self.world                          # drop_last=True on the GLOBAL batch (training)
        return n // gb + (1 if (not self.drop_last and self.world == 1 and n % gb) else 0)

    def steps_to_run(self, args, sw_mask):
        """early-stop rule of train.py:80-92 for this batch (one host sync; the batch is fresh, so nothing can be cached)"""
        from ..train import steps_to_run
        if self.copy_stream is None:
            return steps_to_run(args, sw_mask)
        with torch.cuda.stream(self.copy_stream):           # (sw_mask was produced there: the sync waits for the batch, not for the step in flight)
            return steps_to_run(args, sw_mask)

    def _pinned(self, key, shapes, dtypes, fits=None):
        """the pinned set of `key`, ready to be filled; two per kind (the slots alternate).  A set that does not `fits` is replaced."""
        pin = self._pins.get(key)
        if pin is None or (fits is not None and not fits(pin)):
            pin = self._pins[key] = PinnedSet(shapes, dtypes)
        pin.wait()
        return pin

    def _stage(self, idxs, slot=0):
        """decode one batch into pinned buffers (host side only)"""
        seeds = [self.rng.getrandbits(32) for _ in idxs]
        work = list(zip(idxs, seeds))
        if all(i in self.ds._cache for i in idxs):             # cache hits are index arithmetic: not worth a hand-over to the pool
            items = [self.ds.host_item(i, random.Random(sd)) for i, sd in work]
        else:
            items = list(self.pool.map(lambda a: self.ds.host_item(a[0], random.Random(a[1])), work))
        n, k, S = len(items), self.ds.num_maps, tuple(items[0][0].shape[1:])
        pin = self._pinned((slot & 1, n, S), [(n, 3) + S] + [(n,) + S] * k, [torch.uint8] + [torch.int32] * k)
        for i, it in enumerate(items):
            for view, a in zip(pin.views, it[:1 + k]):
                np.copyto(view[i], a)
        pins = [pin]
        table, layout = self.ds.stage_batch(items, S)
        if table is not None:                                   # one more copy, through a pinned buffer of its own, grown on demand
            tpin = self._pinned(("table", slot & 1), [(max(1024, 2 * len(table)),)], [torch.int64],
                                fits=lambda p: p.tensors[0].numel() >= len(table))
            np.copyto(tpin.views[0][:len(table)], table)
            table = tpin.tensors[0][:len(table)]
            pins.append(tpin)
        mats = None
        if self.ds.augmentation_transform is not None:                      # one matrix per sample, drawn as the reference draws them
            with self._lock:
                mats = torch.stack([self.ds.augmentation_transform.matrix(S[0], S[1]) for _ in items])
        return Staged(pin.tensors[0], pin.tensors[1:], table, layout, mats, pins)

    def _to_device(self, staged):
        """H2D copy, normalisation, warp and target construction of one staged batch -- ALL on the copy stream: none of it depends on the
        training step in flight on the caller's stream, and the host syncs inside (torch.unique, the early-stop rule) then wait for this
        stream only, not for the step (at configs[0]'s batch of 2 the step is 8.6 ms and the serialized batch preparation was ~2 ms of GPU
        idle time per iteration).  The caller's stream waits for the copy stream once, at the end."""
        st = self.copy_stream
        cur = torch.cuda.current_stream()
        mats = staged.mats
        with torch.cuda.stream(st):
            x = staged.image.to(self.device, non_blocking=True)
            maps = [m.to(self.device, non_blocking=True) for m in staged.maps]
            table = None if staged.table is None else staged.table.to(self.device, non_blocking=True)
            for pin in staged.pins:             # the staging sets may be refilled once these copies have run
                pin.record(st)
            maps = self.ds.maps_to_warp(maps, table, staged.layout)
            x = (x.float() / 255.0 - self.mean) / self.std                      # ToTensor + Normalize (train.py:34-37)
            if mats is not None:                                                # dataset.py:66-67: image and maps share one warp
                x = affine_nearest(x, mats)
            warped = []
            for m in maps:
                mf = m.float().unsqueeze(1)
                if mats is not None:
                    mf = affine_nearest(mf, mats)
                warped.append(mf.squeeze(1).round().long())
            ins_d, seg_d = self.ds.label_maps(warped)
            y_mask, y_class, sw_mask, sw_class = targets_from_maps(ins_d, seg_d, self.ds.max_seq_len, device=self.device)
            out = (x.contiguous(), y_mask, y_class, sw_mask, sw_class)
            ign = self.ds.ignore_map(warped)                                    # --ignore_regions: a sixth tensor, (B, N) uint8
            if ign is not None:
                out = out + ((ign != 0).reshape(ign.size(0), -1).to(torch.uint8).contiguous(),)
        cur.wait_stream(st)
        for t in out:                       # allocated on the copy stream, consumed on the caller's: keep the caching allocator from handing
            t.record_stream(cur)            # the blocks to the next batch's side-stream work while the step still reads them
        return out

    def __iter__(self):
        order = list(range(len(self.ds)))
        if self.shuffle:
            self.order_rng.shuffle(order)
        batches = shard_batches(order, self.bs, self.rank, self.world, self.drop_last)
        if not batches:
            return
        staged = self._stage(batches[0], 0)
        for k in range(len(batches)):
            fut, box = None, []
            if k + 1 < len(batches):                                        # decode the next batch while this one trains
                fut = threading.Thread(target=lambda kk=k + 1, out=box: out.append(self._stage(batches[kk], kk)))
                fut.start()
            yield self._to_device(staged)
            if fut is not None:
                fut.join()
                staged = box[0]
