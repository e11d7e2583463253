"""StreetHazards test set from disk for the open-set evaluation (anomaly/dataset.py:40-62,249-300 of the reference,
ValDataset with the DataLoader of eval_ood_traditional.py `main`).

The reference decodes, resizes (Pillow BILINEAR, five scales) and normalises every frame on the host.  Here a pool of
decode threads only runs `Image.open(...).convert('RGB')` / `Image.open(segm)` into a fixed ring of pinned uint8 buffers;
the copy to the device goes on a copy stream, and the compute stream waits on its event before one launch of
dml_pil_resize_normalize writes all scales (bit for bit the reference's tensors, utils/image_resize.py) and
dml_segm_to_label writes `segm - 1`.  `StreetHazardsReader` yields `(img_resized_list, seg_label)` on the device in list
order -- what `eval_ood_traditional.evaluate` consumes.  With `rec_dataset` the image comes from a second tree of
reconstructed frames (dataset.py:255-257,272-273: `rec_dataset/<last folder>/<file name>` of `fpath_img`, resized to the
annotation's size with Pillow NEAREST when it differs); `eval_ood_rec.py` zips such a reader with a plain one.
"""
from __future__ import annotations

import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import utils

IMG_SIZES, IMG_MAX_SIZE, PADDING_CONSTANT = (300, 375, 450, 525, 600), 1000, 8


def default_workers() -> int:
    """decode threads: the CPUs this process may run on, at most 16"""
    return min(16, len(os.sched_getaffinity(0)))


def round2nearest_multiple(x, p):
    return ((x - 1) // p + 1) * p


def resized_shapes(h, w, img_sizes=IMG_SIZES, max_size=IMG_MAX_SIZE, padding=PADDING_CONSTANT):
    """ValDataset's (target_height, target_width) per short side (dataset.py:270-280): short side -> each of img_sizes,
    long side <= max_size, both rounded up to a multiple of padding."""
    out = []
    for short in img_sizes:
        scale = min(short / float(min(h, w)), max_size / float(max(h, w)))
        th, tw = int(h * scale), int(w * scale)
        out.append((round2nearest_multiple(th, padding), round2nearest_multiple(tw, padding)))
    return out


def parse_odgt(odgt, max_sample=-1, start_idx=-1, end_idx=-1):
    """BaseDataset.parse_input_list: a list is taken as is; a path is read as the JSON list on its FIRST line."""
    if isinstance(odgt, list):
        records = odgt
    elif isinstance(odgt, str):
        with open(odgt, "r") as f:
            records = [json.loads(x.rstrip()) for x in f][0]
    else:
        raise TypeError("odgt must be a path or a list of records")
    if max_sample > 0:
        records = records[0:max_sample]
    if start_idx >= 0 and end_idx >= 0:
        records = records[start_idx:end_idx]
    assert len(records) > 0
    return records


class _Slot:
    """One ring entry: pinned host buffers the decoder fills, device buffers the resize reads, and the events that
    order their reuse."""

    def __init__(self, pixels, device):
        self.cap = 0
        self.device = device
        self.copied = torch.cuda.Event()      # H2D done: the pinned buffers may be refilled
        self.consumed = torch.cuda.Event()    # resize done: the device buffers may be overwritten
        self.used = False
        self._alloc(pixels)

    def _alloc(self, pixels):
        self.cap = pixels
        self.h_img = torch.empty(pixels * 3, dtype=torch.uint8).pin_memory()
        self.h_seg = torch.empty(pixels, dtype=torch.uint8).pin_memory()
        self.d_img = torch.empty(pixels * 3, dtype=torch.uint8, device=self.device)
        self.d_seg = torch.empty(pixels, dtype=torch.uint8, device=self.device)

    def ensure(self, pixels):
        """a frame larger than the odgt announced (only then are the buffers replaced)"""
        if pixels > self.cap:
            if self.used:
                self.consumed.synchronize()
            self._alloc(pixels)


class StreetHazardsReader:
    """Iterable over `(img_resized_list, seg_label)` on `device` for every record of the list, in order.
    img_resized_list: fp32 [1, 3, H_s, W_s] per target size; seg_label: int64 [H, W] = annotation - 1."""

    def __init__(self, root_dataset, odgt, img_sizes=IMG_SIZES, img_max_size=IMG_MAX_SIZE,
                 padding_constant=PADDING_CONSTANT, workers=None, device=None, max_sample=-1, rec_dataset=None):
        self.root_dataset = root_dataset
        self.rec_dataset = rec_dataset        # the images of this tree, the annotations of root_dataset (dataset.py:255-260)
        self.records = parse_odgt(odgt, max_sample=max_sample)
        self.img_sizes = tuple(int(s) for s in img_sizes)
        self.img_max_size = img_max_size
        self.padding_constant = padding_constant
        self.workers = int(workers) if workers else default_workers()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.decode_seconds = []              # per frame, as measured in the decode thread

    def __len__(self):
        return len(self.records)

    def sizes(self, h, w):
        return resized_shapes(h, w, self.img_sizes, self.img_max_size, self.padding_constant)

    def _decode(self, rec, slot):
        from PIL import Image
        t0 = time.perf_counter()
        segm = Image.open(os.path.join(self.root_dataset, rec["fpath_segm"]))
        if self.rec_dataset:
            folder_name, image_name = rec["fpath_img"].split("/")[-2:]
            img = Image.open(os.path.join(self.rec_dataset, folder_name, image_name)).convert("RGB")
            if img.size != segm.size:
                img = img.resize(segm.size, Image.NEAREST)           # imresize(img, segm.size, interp='nearest'), :273
        else:
            img = Image.open(os.path.join(self.root_dataset, rec["fpath_img"])).convert("RGB")
        assert segm.mode == "L"
        assert img.size[0] == segm.size[0]
        assert img.size[1] == segm.size[1]
        w, h = img.size
        slot.ensure(h * w)
        np.copyto(slot.h_img[:h * w * 3].numpy().reshape(h, w, 3), np.asarray(img))
        np.copyto(slot.h_seg[:h * w].numpy().reshape(h, w), np.asarray(segm))
        self.decode_seconds.append(time.perf_counter() - t0)
        return h, w

    def __iter__(self):
        recs = self.records
        if not recs:
            return
        dev = self.device
        nslots = min(len(recs), self.workers + 2)
        cap = max(int(r.get("height", 0)) * int(r.get("width", 0)) for r in recs) or 1
        slots = [_Slot(cap, dev) for _ in range(nslots)]
        copy_stream = torch.cuda.Stream(dev)
        compute = torch.cuda.current_stream(dev)
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            futs = {i: pool.submit(self._decode, recs[i], slots[i]) for i in range(nslots)}
            for i in range(len(recs)):
                slot = slots[i % nslots]
                h, w = futs.pop(i).result()
                n = h * w
                with torch.cuda.stream(copy_stream):
                    if slot.used:
                        copy_stream.wait_event(slot.consumed)
                    slot.d_img[:n * 3].copy_(slot.h_img[:n * 3], non_blocking=True)
                    slot.d_seg[:n].copy_(slot.h_seg[:n], non_blocking=True)
                    slot.copied.record(copy_stream)
                compute.wait_event(slot.copied)
                imgs = utils.pil_resize_normalize(slot.d_img[:n * 3].view(h, w, 3), self.sizes(h, w))
                seg_label = utils.segm_to_label(slot.d_seg[:n].view(h, w))
                slot.consumed.record(compute)
                slot.used = True
                nxt = i + nslots
                if nxt < len(recs):
                    slot.copied.synchronize()         # the pinned buffers are free once the copy has landed
                    futs[nxt] = pool.submit(self._decode, recs[nxt], slot)
                yield imgs, seg_label
