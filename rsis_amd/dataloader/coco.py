"""COCO reader: a standard `instances_<set>.json` read for training and evaluation, on the base class of reader.py and the device
loader of loader.py.  The reference has no COCO reader (its datasets are Pascal VOC, Cityscapes and CVPPP); the sample pipeline is
Pascal's (dataset.py:47-84, dataset_utils.py:27-57) with the label images replaced by the file's polygons:
  host   : the annotation file, parsed ONCE into flat numpy arrays (below); JPEG decode and the PIL bilinear `Scale` of the image;
           the flip / crop draws and the decode cache are Reader's.  Instead of label arrays (`num_maps` = 0) `host_item` returns a
           small record (sample, resized size, flip, crop offsets); `stage_batch` = `stage_tables` turns the batch's records into ONE
           int64 table: the polygons at their native sizes and two index tables per sample, src_y / src_x, that fold the nearest
           resize, the flip and the crop of the maps;
  device : `maps_to_warp` = `device_maps`: one rsis_poly_to_bits launch for all records of the batch (polymask.hip, bit for bit the
           COCO mask API), one rsis_paint_instance_maps launch (cocomaps.hip) that writes the instance-id and class-id maps at the
           output size; then, as for Pascal, normalisation, ONE affine warp shared by image and maps, the targets
           (rsis_targets_from_maps).
The label images never exist on the host, nor at native size anywhere.

Parsing rules (also INTEGRATION.md):
  classes   : ["<eos>"] + the category names in ascending category-id order; class index = 1 + rank of the category id.  A
              -num_classes other than len(classes) raises and names the right value.
  crowd     : `iscrowd` records are never painted as instances.  Without --ignore_regions their pixels stay background.  With it they
              make the batch's IGNORE MAP (the loader's sixth tensor, left out of the mask loss): records stored as uncompressed run
              counts or as polygons go to bit rows with the launches cocoeval uses (rsis_rle_to_bits / rsis_poly_to_bits), and one
              rsis_paint_ignore_map launch writes the uint8 map at the output size through the same src_y / src_x tables: 1 where any
              crowd record covers the pixel and no instance was painted there (an outlined instance inside a crowd still counts).  The
              map is warped with the image and the label maps (fill outside the frame: 0 = counted).  At most MAX_CROWDS = 16 crowd
              records per image: beyond that the 16 largest by the file's `area` are kept, with one warning per run.  A crowd record in
              another form (compressed RLE text, counts that do not add up to the image) is skipped and counted in that warning.
  kind      : a record whose segmentation is not polygons (cocoeval.segmentation_kind: RLE of a non-crowd record, a bare box, a broken
              part) is skipped; one warning per run says how many.
  images    : an image with no paintable record is left out of the sample list; the count is printed once.
  cap       : more than 255 paintable records in an image keep the 255 largest by the file's `area` field (ties: file order).  The
              kept records get the instance ids 1..k in file order.
  overlap   : a pixel under several records belongs to the one of the smallest MASK area (equal areas: the earlier record), so that a
              small object lying on a large one stays visible.
  resize    : scipy.ndimage.zoom(order=0, mode='nearest'), what the other readers apply to their maps, from native length n to length m
              reads index floor(o * ((n - 1) / (m - 1)) + 0.5) in float64 (index 0 for m == 1): `zoom_index`.
Inherited quirk: sequence_from_masks / rsis_targets_from_maps drop the smallest id PRESENT as the background, so a crop without one
background pixel loses its instance 1 -- as in the reference's readers.
Memory: the parsed file is a float64 array of all kept vertices plus int64 / int32 offset arrays (16 bytes per vertex); the JSON tree
itself is released after parsing.  The footprint on instances_train2017.json has not been measured."""
import json
import os
import sys

import numpy as np
import torch

from .reader import Reader, flip_crop, scale_image

MAX_RECORDS = 255          # instance ids of rsis_targets_from_maps: 0..255
MAX_CROWDS = 16            # crowd records of one image that make its ignore map (--ignore_regions); COCO images carry one or two


def zoom_index(n, m):
    """(m,) int32: the input index that scipy.ndimage.zoom(order=0, mode='nearest') reads for each of the m outputs of an axis of
    native length n"""
    n, m = int(n), int(m)
    if m <= 1:
        return np.zeros((max(m, 0),), np.int32)
    o = np.arange(m, dtype=np.float64)
    return np.floor(o * (np.float64(n - 1) / np.float64(m - 1)) + 0.5).astype(np.int32)


def index_tables(native, resized, flip=False, crop=None, size=None):
    """(src_y, src_x) int32: the native row / column under every output row / column after the nearest resize native -> resized, the
    horizontal flip and the crop (oh, ow) of `size` = (S, S)"""
    sy, sx = zoom_index(native[0], resized[0]), zoom_index(native[1], resized[1])
    if flip:
        sx = sx[::-1]
    if crop is not None:
        sy, sx = sy[crop[0]:crop[0] + size[0]], sx[crop[1]:crop[1] + size[1]]
    return np.ascontiguousarray(sy), np.ascontiguousarray(sx)


def polygon_mask(parts, h, w):
    """one polygon record -> (h, w) uint8 on the host: the rule of rsis_amd/csrc/polymask.hip in numpy (prefix parity, in column-major
    element order, of the boundary positions the 5x edge walk toggles; the union of the parts).  For get_raw_sample and
    tools/bench_cocomaps.py only: the loader rasterises on the device."""
    out = np.zeros((h * w,), np.uint8)
    for part in parts:
        p = np.asarray(part, np.float64).reshape(-1, 2)
        x, y = (5.0 * p[:, 0] + .5).astype(np.int64), (5.0 * p[:, 1] + .5).astype(np.int64)
        us, vs = [], []
        for j in range(len(x)):
            xs, xe, ys, ye = int(x[j]), int(x[(j + 1) % len(x)]), int(y[j]), int(y[(j + 1) % len(x)])
            dx, dy = abs(xe - xs), abs(ys - ye)
            rev = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
            if rev:
                xs, xe, ys, ye = xe, xs, ye, ys
            d = np.arange(max(dx, dy) + 1, dtype=np.int64)
            t = (max(dx, dy) - d) if rev else d
            if dx >= dy:
                us.append(t + xs)
                vs.append(np.zeros_like(t) if dx == 0 else
                          ((np.float64(ys) + (np.float64(ye - ys) / np.float64(dx)) * t.astype(np.float64)) + .5).astype(np.int64))
            else:
                vs.append(t + ys)
                us.append(((np.float64(xs) + (np.float64(xe - xs) / np.float64(dy)) * t.astype(np.float64)) + .5).astype(np.int64))
        u, v = np.concatenate(us), np.concatenate(vs)
        u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
        xd = (np.where(u1 < u0, u1, u1 - 1).astype(np.float64) + .5) / 5.0 - .5
        ok = (u1 != u0) & (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
        yd = np.ceil(np.clip((np.minimum(v1, v0).astype(np.float64) + .5) / 5.0 - .5, 0.0, float(h)))
        pos = xd[ok].astype(np.int64) * h + yd[ok].astype(np.int64)
        pos = pos[pos < h * w]
        out |= (np.cumsum(np.bincount(pos, minlength=h * w) & 1) & 1).astype(np.uint8)
    return np.ascontiguousarray(out.reshape(w, h).T)


def compose_maps(masks, inst_ids, class_ids, h, w):
    """(ins, seg) int32 (h, w) from the records' masks by the rule of rsis_paint_instance_maps: smallest mask area wins, ties to the
    lower index, a mask of area 0 never wins"""
    ins, seg = np.zeros((h, w), np.int32), np.zeros((h, w), np.int32)
    best = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    for m, i, c in zip(masks, inst_ids, class_ids):
        a = int(m.sum())
        take = (m > 0) & (a < best)
        if a > 0:
            ins[take], seg[take], best[take] = i, c, a
    return ins, seg


class COCO(Reader):
    """A COCO instances file behind the readers' interface: same constructor arguments, `classes`, `get_classes`, `get_sample_list`,
    `__len__`, `get_raw_sample`, `image_path`, `raw_size`; `host_item` returns (image, record) and the loader paints both maps on the
    device (`stage_tables` on its staging thread, `device_maps` on its copy stream)"""
    num_maps = 0
    has_ignore_source = True    # iscrowd records: --ignore_regions

    def __init__(self, args, transform=None, target_transform=None, augment=False, split="train", resize=False, imsize=256):
        if split not in ("train", "val"):
            raise ValueError("-dataset coco has the splits train and val (the test sets have no annotations), not %r" % (split,))
        self._setup(args, transform, target_transform, augment, split, resize, imsize, crop=args.batch_size != 1,
                    zoom_range=(args.zoom, max(args.zoom * 2, 1.0)))       # the augmentation of pascal.py:46-51
        name = args.coco_train_set if split == "train" else args.coco_val_set
        self.ann_file = os.path.join(args.coco_dir, "annotations", "instances_%s.json" % name)
        self.image_dir = os.path.join(args.coco_dir, name)
        self._parse()
        self.num_classes = len(self.classes)
        if int(args.num_classes) != self.num_classes:
            raise ValueError("%s has %d categories: -num_classes must be %d (the categories and <eos>), not %d"
                             % (self.ann_file, self.num_classes - 1, self.num_classes, int(args.num_classes)))

    # ------------------------------------------------------------------ the annotation file ------------------------------------------
    def _parse(self):
        from ..cocoeval import segmentation_kind
        with open(self.ann_file) as f:
            d = json.load(f)
        cats = sorted(d["categories"], key=lambda c: c["id"])
        self.classes = ["<eos>"] + [c["name"] for c in cats]
        self.category_ids = [0] + [c["id"] for c in cats]                  # class index -> the file's category id
        class_of = {c["id"]: k + 1 for k, c in enumerate(cats)}
        images = d["images"]
        pos = {im["id"]: k for k, im in enumerate(images)}
        per_image = [[] for _ in images]                                    # paintable records of every image, in file order
        crowd_of = [[] for _ in images]                                     # --ignore_regions: (area, kind, data) of its crowd records
        skipped = crowd_skipped = crowd_capped = 0
        for ann in d["annotations"]:
            if ann.get("iscrowd", 0):
                if self.ignore_regions and ann["image_id"] in pos:
                    rec = self._crowd_record(ann, images[pos[ann["image_id"]]], segmentation_kind)
                    if rec is None:
                        crowd_skipped += 1
                    else:
                        crowd_of[pos[ann["image_id"]]].append(rec)
                continue
            try:
                kind = segmentation_kind(ann.get("segmentation"))
            except ValueError:
                kind = None
            if kind != "polygons" or ann["image_id"] not in pos or ann["category_id"] not in class_of:
                skipped += 1
                continue
            per_image[pos[ann["image_id"]]].append(ann)
        if skipped:
            print("warning: %s: %d records without a polygon segmentation (or of an unknown image / category) are skipped"
                  % (self.ann_file, skipped), file=sys.stderr)
        ids, files, sizes, rec_off, part_off, vert_off, xy, cls = [], [], [], [0], [0], [0], [], []
        self.crowds = []                                                    # sample -> [(kind, data)], at most MAX_CROWDS
        for im, anns, crowds in zip(images, per_image, crowd_of):
            if not anns:                                                    # (an image whose only records are crowds stays left out)
                continue
            if len(crowds) > MAX_CROWDS:                                    # the largest by `area` (stable: ties in file order)
                order = np.argsort(-np.asarray([c[0] for c in crowds], np.float64), kind="stable")[:MAX_CROWDS]
                crowds = [crowds[k] for k in sorted(order.tolist())]
                crowd_capped += 1
            self.crowds.append([c[1:] for c in crowds])
            if len(anns) > MAX_RECORDS:                                     # the 255 largest by `area` (stable: ties in file order)
                order = np.argsort(-np.asarray([float(a.get("area", 0.0)) for a in anns], np.float64), kind="stable")[:MAX_RECORDS]
                anns = [anns[k] for k in sorted(order.tolist())]
            ids.append(im["id"])
            files.append(im["file_name"])
            sizes.append((int(im["height"]), int(im["width"])))
            for ann in anns:
                for part in ann["segmentation"]:
                    v = np.asarray(part, dtype=np.float64)
                    xy.append(v)
                    vert_off.append(vert_off[-1] + len(v) // 2)
                part_off.append(len(vert_off) - 1)
                cls.append(class_of[ann["category_id"]])
            rec_off.append(len(cls))
        if crowd_skipped or crowd_capped:
            print("warning: %s: --ignore_regions: %d crowd records in a form other than run counts or polygons are skipped; %d images "
                  "have more than %d crowd records (the largest by area are kept)" % (self.ann_file, crowd_skipped, crowd_capped, MAX_CROWDS),
                  file=sys.stderr)
        left_out = len(images) - len(ids)
        if left_out:
            print("%s: %d of %d images have no paintable record and are left out" % (self.ann_file, left_out, len(images)))
        self.image_ids = ids
        self.image_files = [os.path.join(self.image_dir, f) for f in files]
        self.native_size = np.asarray(sizes, np.int64).reshape(-1, 2)
        self.rec_off = np.asarray(rec_off, np.int64)                        # sample -> its records
        self.part_off = np.asarray(part_off, np.int64)                      # record -> its parts
        self.vert_off = np.asarray(vert_off, np.int64)                      # part -> its vertices
        self.xy = np.concatenate(xy) if xy else np.zeros((0,), np.float64)  # (x, y) pairs of every kept part
        self.rec_class = np.asarray(cls, np.int32)

    @staticmethod
    def _crowd_record(ann, im, segmentation_kind):
        """(area, kind, data) of a crowd record that can make an ignore region, or None: 'counts' -> uint32 run counts that add up to
        the image, 'polygons' -> list of float64 parts"""
        seg = ann.get("segmentation")
        try:
            kind = segmentation_kind(seg)
        except ValueError:
            return None
        area = float(ann.get("area", 0.0))
        if kind == "polygons":
            return area, kind, [np.asarray(p, dtype=np.float64) for p in seg]
        if kind == "counts":
            h, w = int(im["height"]), int(im["width"])
            c = np.asarray(seg["counts"], dtype=np.int64)
            if [int(v) for v in seg["size"]] != [h, w] or (c < 0).any() or int(c.sum()) != h * w or len(c) == 0:
                return None
            return area, kind, c.astype(np.uint32)
        return None

    def raw_size(self, index):
        """(height, width) of the original image, as the annotation file states it"""
        return int(self.native_size[index, 0]), int(self.native_size[index, 1])

    def records(self, index):
        """[(parts: list of float64 (2k,) views, instance id, class index)] of a sample"""
        out = []
        for k, r in enumerate(range(int(self.rec_off[index]), int(self.rec_off[index + 1]))):
            parts = [self.xy[2 * int(self.vert_off[p]):2 * int(self.vert_off[p + 1])]
                     for p in range(int(self.part_off[r]), int(self.part_off[r + 1]))]
            out.append((parts, k + 1, int(self.rec_class[r])))
        return out

    def get_raw_sample(self, index):
        """(PIL RGB image, instance-id map, class map) in raw size, the maps composed in numpy (API parity; the loader never calls it)"""
        from PIL import Image
        img = Image.open(self.image_path(index)).convert("RGB")
        h, w = self.raw_size(index)
        recs = self.records(index)
        ins, seg = compose_maps([polygon_mask(p, h, w) for p, _i, _c in recs], [i for _p, i, _c in recs], [c for _p, _i, c in recs], h, w)
        return img, ins, seg

    # ------------------------------------------------------------------ per sample, on the host --------------------------------------
    def _decode(self, index):
        from PIL import Image
        return (scale_image(Image.open(self.image_path(index)).convert("RGB"), self.imsize, self.resize),)

    def host_item(self, index, rng):
        """-> (uint8 image (3, S, S), record): record = (sample, resized (h, w), flip, crop (oh, ow) or None); the draws are Reader's"""
        im, = self._decoded(index)
        h, w = im.shape[1:]
        flip, crop = self._draw((h, w), rng)
        return np.ascontiguousarray(flip_crop(im, flip, crop, self.imsize)), (int(index), (h, w), flip, crop)

    # ------------------------------------------------------------------ per batch: tables on the host, maps on the device -------------
    def stage_tables(self, records, S):
        """the batch's records -> (table: int64 numpy array, layout): the polygons of every sample at native size and the index tables,
        concatenated for ONE host-to-device copy.  Sections, in int64 words: xy (float64 bits) | parts[np][2] | poly recs[n][8] |
        paint recs[n][8] | imgs[B][2] | src_y[B][Ho] and src_x[B][Wo] (int32 pairs)."""
        from ..cocoeval import words_of
        B, (Ho, Wo) = len(records), S
        r0 = np.asarray([self.rec_off[r[0]] for r in records], np.int64)
        r1 = np.asarray([self.rec_off[r[0] + 1] for r in records], np.int64)
        cnt = r1 - r0
        rec = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in zip(r0, r1)])          # dataset record of every batch record
        n = len(rec)
        sample = np.repeat(np.arange(B), cnt)
        hw = self.native_size[[r[0] for r in records]][sample]                                    # (n, 2) native sizes
        nparts = self.part_off[rec + 1] - self.part_off[rec]
        part = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in zip(self.part_off[rec], self.part_off[rec + 1])])
        nverts = self.vert_off[part + 1] - self.vert_off[part]
        xy = np.concatenate([self.xy[2 * a:2 * b] for a, b in zip(self.vert_off[part], self.vert_off[part + 1])])
        words = 2 * ((hw[:, 0] * hw[:, 1] + 127) // 128)                                         # cocoeval.words_of
        assert n == 0 or int(words[0]) == words_of(int(hw[0, 0] * hw[0, 1]))
        first_word = np.cumsum(words) - words
        ptab = np.stack([np.cumsum(nverts) - nverts, nverts], axis=1)
        zero = np.zeros((n,), np.int64)
        poly = np.stack([np.cumsum(nparts) - nparts, nparts, hw[:, 0], hw[:, 1], first_word, words, zero, zero], axis=1)
        iid = np.concatenate([np.arange(1, c + 1, dtype=np.int64) for c in cnt])
        paint = np.stack([first_word, words, hw[:, 0], hw[:, 1], iid, self.rec_class[rec].astype(np.int64), zero, zero], axis=1)
        imgs = np.stack([np.cumsum(cnt) - cnt, cnt], axis=1)
        src = np.zeros((2 * ((B * (Ho + Wo) + 1) // 2),), np.int32)
        for b, (index, resized, flip, crop) in enumerate(records):
            sy, sx = index_tables(self.native_size[index], resized, flip, crop, S)
            src[b * Ho:(b + 1) * Ho] = sy
            src[B * Ho + b * Wo:B * Ho + (b + 1) * Wo] = sx
        secs = [xy.view(np.int64), ptab.reshape(-1), poly.reshape(-1), paint.reshape(-1), imgs.reshape(-1), src.view(np.int64)]
        crowd = None
        if self.ignore_regions:
            csecs, crowd = self._stage_crowds(records)
            secs += csecs
        off = np.concatenate([[0], np.cumsum([len(s) for s in secs])])
        layout = dict(off=[int(v) for v in off], nverts=int(nverts.sum()), nparts=len(part), n=n, B=B, Ho=int(Ho), Wo=int(Wo),
                      words=int(words.sum()), max_recs=int(cnt.max()), crowd=crowd)
        return np.concatenate(secs), layout

    def _stage_crowds(self, records):
        """the crowd records of the batch -> (seven more int64 sections, their layout): polygon xy | parts[np][2] | poly recs[npoly][8] |
        run counts (uint32 pairs) | rle desc[nrle][4] | crowd recs[nc][8] (first word, words, h, w) | imgs[B][2].  The bit rows of the
        run-count records come first in the crowd bit buffer, those of the polygon records after them."""
        from ..cocoeval import words_of
        xy, ptab, prec, counts, desc, crec, imgs = [], [], [], [], [], [], []
        nv = ncount = 0
        rle_words = sum(words_of(int(self.native_size[r[0], 0] * self.native_size[r[0], 1]))
                        for r in records for kind, _d in self.crowds[r[0]] if kind == "counts")
        rle_at, poly_at = 0, 0
        for index, _resized, _flip, _crop in records:
            h, w = int(self.native_size[index, 0]), int(self.native_size[index, 1])
            nw = words_of(h * w)
            imgs.append((len(crec), len(self.crowds[index])))
            for kind, data in self.crowds[index]:
                if kind == "counts":
                    desc.append((ncount, len(data), rle_at, nw))
                    counts.append(data)
                    ncount += len(data)
                    crec.append((rle_at, nw, h, w, 0, 0, 0, 0))
                    rle_at += nw
                else:
                    prec.append((len(ptab), len(data), h, w, poly_at, nw, 0, 0))
                    for part in data:
                        ptab.append((nv, len(part) // 2))
                        xy.append(part)
                        nv += len(part) // 2
                    crec.append((rle_words + poly_at, nw, h, w, 0, 0, 0, 0))
                    poly_at += nw
        allc = np.concatenate(counts + [np.zeros((1 + (ncount + 1) % 2,), np.uint32)]).astype(np.uint32)     # (never empty, an even length)
        i64 = lambda rows, k: np.asarray(rows, np.int64).reshape(-1, k).reshape(-1)      # noqa: E731
        secs = [(np.concatenate(xy) if xy else np.zeros((0,), np.float64)).view(np.int64), i64(ptab, 2), i64(prec, 8), allc.view(np.int64),
                i64(desc, 4), i64(crec, 8), i64(imgs, 2)]
        lay = dict(nverts=nv, nparts=len(ptab), npoly=len(prec), ncounts=int(len(allc)), nrle=len(desc), n=len(crec),
                   rle_words=int(rle_words), poly_words=int(poly_at), max_recs=max([c for _f, c in imgs] + [0]))
        return secs, lay

    def stage_batch(self, items, S):
        return self.stage_tables([it[1] for it in items], S)

    def maps_to_warp(self, maps, table, layout):
        ins, seg = self.device_maps(table, layout)
        if not self.ignore_regions:
            return [ins, seg]
        return [ins, seg, self.device_ignore_map(table, layout, ins).to(torch.int32)]       # the map is warped as one more map

    def label_maps(self, maps):
        return maps[0], maps[1]

    def ignore_map(self, maps):
        return maps[2] if self.ignore_regions else None

    @staticmethod
    def device_ignore_map(table, layout, ins):
        """table / layout of stage_tables under --ignore_regions, ins: the painted instance map -> (B, Ho, Wo) uint8 ignore map: at most
        three launches on the current stream (run counts -> bits, polygons -> bits, the paint), no sync"""
        from .._lib import check, lib, ptr, stream
        L, o, c, dev = lib(), layout["off"], layout["crowd"], table.device
        B, Ho, Wo = layout["B"], layout["Ho"], layout["Wo"]
        ign = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev)       # every element is written by the kernel
        xy, ptab, prec, counts, desc, crec, imgs = (table[o[k]:o[k + 1]] for k in range(6, 13))
        nw = c["rle_words"] + c["poly_words"]
        bits = torch.empty((max(nw, 1),), dtype=torch.int64, device=dev)
        if c["nrle"]:
            cd = counts.view(torch.int32)
            ends, area = torch.empty_like(cd), torch.empty((c["nrle"],), dtype=torch.int32, device=dev)
            check(L.rsis_rle_to_bits(ptr(cd), cd.numel(), ptr(desc), c["nrle"], ptr(ends), ptr(bits), c["rle_words"], ptr(area), stream()),
                  "rsis_rle_to_bits")
        if c["npoly"]:
            scratch = torch.empty((c["poly_words"],), dtype=torch.int64, device=dev)
            area = torch.empty((c["npoly"],), dtype=torch.int32, device=dev)
            check(L.rsis_poly_to_bits(ptr(xy), c["nverts"], ptr(ptab), c["nparts"], ptr(prec), c["npoly"], ptr(scratch),
                                      ptr(bits) + 8 * c["rle_words"], c["poly_words"], ptr(area), stream()), "rsis_poly_to_bits")
        src = table[o[5]:o[6]].view(torch.int32)
        check(L.rsis_paint_ignore_map(ptr(bits) if c["n"] else None, nw, c["n"], ptr(crec) if c["n"] else None, ptr(imgs), B, c["max_recs"],
                                      ptr(src), ptr(src) + 4 * B * Ho, Ho, Wo, ptr(ins), ptr(ign), stream()), "rsis_paint_ignore_map")
        return ign

    @staticmethod
    def device_maps(table, layout):
        """table: the int64 CUDA tensor of stage_tables -> (ins, seg) int32 (B, Ho, Wo): two launches on the current stream, no sync"""
        from .._lib import check, lib, ptr, stream
        L, o, dev = lib(), layout["off"], table.device
        B, Ho, Wo, n, nw = layout["B"], layout["Ho"], layout["Wo"], layout["n"], layout["words"]
        xy, ptab, poly, paint, imgs = (table[o[k]:o[k + 1]] for k in range(5))
        src = table[o[5]:o[6]].view(torch.int32)
        scratch = torch.empty((nw,), dtype=torch.int64, device=dev)
        bits = torch.empty((nw,), dtype=torch.int64, device=dev)
        area = torch.empty((n,), dtype=torch.int32, device=dev)
        ins = torch.empty((B, Ho, Wo), dtype=torch.int32, device=dev)       # every element is written by the kernel
        seg = torch.empty((B, Ho, Wo), dtype=torch.int32, device=dev)
        check(L.rsis_poly_to_bits(ptr(xy), layout["nverts"], ptr(ptab), layout["nparts"], ptr(poly), n, ptr(scratch), ptr(bits), nw,
                                  ptr(area), stream()), "rsis_poly_to_bits")
        check(L.rsis_paint_instance_maps(ptr(bits), nw, ptr(area), n, ptr(paint), ptr(imgs), B, layout["max_recs"], ptr(src),
                                         ptr(src) + 4 * B * Ho, Ho, Wo, ptr(ins), ptr(seg), stream()), "rsis_paint_instance_maps")
        return ins, seg


def _runs(mask):
    """(h, w) 0/1 -> uncompressed COCO counts: run lengths in column-major order, starting with the run of zeros"""
    v = np.asarray(mask, np.uint8).T.reshape(-1)
    edges = np.flatnonzero(np.diff(v)) + 1
    counts = np.diff(np.concatenate([[0], edges, [len(v)]])).tolist()
    return ([0] if v[0] else []) + [int(c) for c in counts]


def synthesize_coco_dir(path, n=6, sizes=((48, 64), (75, 50), (33, 47)), seed=0, sets=("train2017", "val2017")):
    """Write a small COCO-shaped tree: <set>/NNNNNNNNNNNN.jpg and annotations/instances_<set>.json for each of `sets`, with the sparse
    category ids 3, 17, 44.  Each set has n annotated images (image i of size sizes[i % len(sizes)], (height, width)) whose records are,
    in file order: a large quadrilateral, a small triangle nested in it, a twelve-gon that overlaps the quadrilateral, a record of two
    separate parts, and two congruent overlapping rectangles (equal areas); image 0 also carries a crowd record as uncompressed
    counts.  Two more images follow: one with only a crowd record and one with no record.  Coordinates are fractional.  For tests and
    smoke runs of the data path only."""
    from PIL import Image
    os.makedirs(os.path.join(path, "annotations"), exist_ok=True)
    r = np.random.default_rng(seed)
    cats = [{"id": 3, "name": "car", "supercategory": "vehicle"}, {"id": 17, "name": "cat", "supercategory": "animal"},
            {"id": 44, "name": "bottle", "supercategory": "kitchen"}]

    def area_of(part):
        p = np.asarray(part, np.float64).reshape(-1, 2)
        return float(abs(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])) / 2.0)

    for si, name in enumerate(sets):
        os.makedirs(os.path.join(path, name), exist_ok=True)
        images, anns = [], []
        for i in range(n + 2):
            H, W = sizes[i % len(sizes)]
            img_id = 1000 * (si + 1) + 7 * i + 3
            rgb = r.integers(0, 70, (H, W, 3)).astype(np.uint8)
            segs = []                                                        # (category id, segmentation, iscrowd)
            if i < n:
                j = r.uniform(0.0, 1.5, 8)
                quad = [0.08 * W + j[0], 0.10 * H + j[1], 0.80 * W + j[2], 0.06 * H + j[3], 0.86 * W - j[4], 0.82 * H - j[5],
                        0.05 * W + j[6], 0.75 * H - j[7]]
                tri = [0.30 * W + j[0], 0.30 * H, 0.50 * W + 0.25, 0.32 * H + j[1], 0.40 * W, 0.55 * H + 0.5]
                th = np.arange(12) * (2 * np.pi / 12)
                gon = np.stack([0.70 * W + 0.28 * W * np.cos(th), 0.60 * H + 0.30 * H * np.sin(th)], axis=1)
                gon = np.clip(gon, 0.0, [W, H]).reshape(-1).tolist()
                two = [[0.02 * W, 0.85 * H, 0.20 * W + 0.5, 0.85 * H, 0.20 * W + 0.5, 0.98 * H, 0.02 * W, 0.98 * H],
                       [0.55 * W, 0.02 * H + 0.25, 0.75 * W, 0.02 * H + 0.25, 0.65 * W, 0.20 * H]]
                x0, y0, a, b = 0.10 * W + 0.5, 0.40 * H + 0.5, int(0.25 * W), int(0.2 * H)
                rect = lambda dx, dy: [x0 + dx, y0 + dy, x0 + dx + a, y0 + dy, x0 + dx + a, y0 + dy + b, x0 + dx, y0 + dy + b]   # noqa: E731
                segs = [(3, [quad], 0), (17, [tri], 0), (44, [gon], 0), (17, two, 0), (3, [rect(0, 0)], 0), (44, [rect(a // 2, 3)], 0)]
                for k, (_c, seg, _cr) in enumerate(segs):
                    for part in seg:
                        p = np.asarray(part).reshape(-1, 2)
                        xa, xb, ya, yb = [int(v) for v in (p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max())]
                        rgb[ya:yb, xa:xb] = (60 + 30 * k, 250 - 35 * k, 90 + 25 * (k % 3))
            if i == 0 or i == n:                                             # a crowd region as uncompressed run counts
                m = np.zeros((H, W), np.uint8)
                m[H // 2:H // 2 + H // 4, W // 3:W // 3 + W // 3] = 1
                segs.append((3, {"size": [H, W], "counts": _runs(m)}, 1))
            fname = "%012d.jpg" % img_id
            Image.fromarray(rgb).save(os.path.join(path, name, fname), quality=90)
            images.append({"id": img_id, "file_name": fname, "height": H, "width": W})
            for cat, seg, crowd in segs:
                if crowd:
                    area, xs, ys = float(sum(seg["counts"][1::2])), [W // 3, W // 3 + W // 3], [H // 2, H // 2 + H // 4]
                else:
                    area = sum(area_of(p) for p in seg)
                    pts = np.concatenate([np.asarray(p).reshape(-1, 2) for p in seg])
                    xs, ys = [pts[:, 0].min(), pts[:, 0].max()], [pts[:, 1].min(), pts[:, 1].max()]
                anns.append({"id": 100000 * (si + 1) + len(anns) + 1, "image_id": img_id, "category_id": cat, "segmentation": seg,
                             "area": area, "bbox": [float(xs[0]), float(ys[0]), float(xs[1] - xs[0]), float(ys[1] - ys[0])],
                             "iscrowd": crowd})
        with open(os.path.join(path, "annotations", "instances_%s.json" % name), "w") as f:
            json.dump({"info": {"description": "synthetic"}, "licenses": [], "images": images, "annotations": anns, "categories": cats}, f)
    return path
