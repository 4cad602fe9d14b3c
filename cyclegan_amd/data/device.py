"""Device-resident input pipeline.

Same public surface and the same sample order as ``Pipeline``, but the
dataset lives on the device as raw uint8 (horse2zebra: 2,661 images x
196,608 B ~ 0.5 GB) and every batch is produced by ONE augmentation kernel
(ops.augment.augment_batch) — straight into the captured graph's static
input buffers when ``train_epoch(epoch, out=(sx, sy))`` is given them. Per
step there is no host tensor work, no pinned allocation and no H2D image
traffic: the epoch's shuffled index list is uploaded once and each step's
``idx`` is a view into it.

augment="frozen" draws every train sample's (flip, oy, ox) once, from the
same generator in the same order as ``Pipeline.__init__`` — each sample gets
exactly the augmentation ``Pipeline`` would have cached (the reference's
.map().cache()). augment="epoch" re-draws them at the start of every epoch,
which costs nothing here.

One image size per split is required (a single [N,H,W,3] tensor); folders
of mixed sizes stay on the host ``Pipeline``.
"""

from __future__ import annotations

import math
import os
from typing import List, Optional, Tuple

import torch

from ..ops.augment import augment_batch, make_idx, make_params
from .pipeline import (SPLITS, ShuffleBuffer, draw_train_params,
                       folder_image_names, load_raw, resize_shape)

# offset of the per-epoch augmentation stream from the shuffle stream
# (seed * 100003 + epoch): far above any shuffle seed in use
_AUG_STREAM = 1 << 62


def _stack_split(name: str, imgs: List[torch.Tensor], data_dir) -> torch.Tensor:
    for i, im in enumerate(imgs):
        if im.shape != imgs[0].shape:
            where = name
            if data_dir:
                d = os.path.join(data_dir, name)
                where = os.path.join(d, folder_image_names(d)[i])
            raise ValueError(
                f"device pipeline needs one image size per split: {where} is "
                f"{tuple(im.shape[:2])}, the split's first image is "
                f"{tuple(imgs[0].shape[:2])}; use the host pipeline "
                f"(--data_device host) for mixed sizes")
    return torch.stack(imgs)


class DevicePipeline:
    def __init__(self, args, ctx, image_size: int = 256,
                 augment: str = "frozen",
                 device: Optional[torch.device] = None,
                 dtype: Optional[torch.dtype] = None):
        if augment not in ("frozen", "epoch"):
            raise ValueError(f"augment must be 'frozen' or 'epoch', got {augment!r}")
        self.ctx = ctx
        self.global_batch = args.global_batch_size
        self.per_replica = args.batch_size
        self.image_size = image_size
        self.seed = getattr(args, "seed", 1234)
        self.augment = augment
        self.device = torch.device(device if device is not None else ctx.device)
        # the trainer's compute dtype rule (trainer.CycleGAN.__init__)
        self.dtype = dtype or getattr(args, "compute_dtype", None) or (
            torch.bfloat16 if self.device.type == "cuda" else torch.float32)

        data_dir = getattr(args, "data_dir", None)
        raw = load_raw(args, image_size, self.seed)
        self.num_train = min(len(raw["trainA"]), len(raw["trainB"]))
        self.num_test = min(len(raw["testA"]), len(raw["testB"]))
        self.train_steps = math.ceil(self.num_train / self.global_batch)
        self.test_steps = math.ceil(self.num_test / self.global_batch)

        self.resize_hw = resize_shape(image_size)
        self.crop_hw = (image_size, image_size)

        # one upload per split, raw bytes
        n = {"trainA": self.num_train, "trainB": self.num_train,
             "testA": self.num_test, "testB": self.num_test}
        self.src = {s: _stack_split(s, raw[s], data_dir)[: n[s]].to(self.device)
                    for s in SPLITS}

        if augment == "frozen":
            self._train_params = self._upload_params(self.draw_params(
                torch.Generator().manual_seed(self.seed)))
        # test data: no flip, no offset, resize == crop
        zeros = [[0, 0, 0]] * self.num_test
        self._test_params = make_params(zeros, self.crop_hw, self.crop_hw,
                                        self.device)
        self._test_idx = make_idx(range(self.num_test), max(self.num_test, 1),
                                  self.device)

    # ---- augmentation parameters ----

    def draw_params(self, gen: torch.Generator):
        """Host [N,3] (flip, oy, ox) for all of trainA, then all of trainB —
        the order Pipeline.__init__ draws in."""
        out = []
        for s in ("trainA", "trainB"):
            hw = tuple(self.src[s].shape[1:3])
            out.append(torch.tensor(
                [draw_train_params(gen, hw, self.resize_hw, self.crop_hw)
                 for _ in range(self.num_train)],
                dtype=torch.int64).reshape(-1, 3))
        return out

    def epoch_params(self, epoch: int):
        """augment="epoch": the draw of one epoch, a function of (seed,
        epoch) only — the same on every rank, on a stream of its own."""
        g = torch.Generator().manual_seed(
            _AUG_STREAM + self.seed * 100003 + epoch)
        return self.draw_params(g)

    def _upload_params(self, host_params):
        # range-checked on the host, then uploaded
        return [make_params(p, self.resize_hw, self.crop_hw, self.device)
                for p in host_params]

    # ---- batches ----

    def _rank_range(self, lo: int, hi: int) -> Tuple[int, int]:
        """Positions [lo, hi) of a global batch -> this rank's slice of it
        (Pipeline._rank_slice on positions; may be empty)."""
        r, b = self.ctx.rank, self.per_replica
        return min(lo + r * b, hi), min(lo + (r + 1) * b, hi)

    def _batch(self, split, idx, params, resize_hw, out=None):
        if idx.shape[0] != self.per_replica:
            out = None  # short batches always get fresh tensors
        return augment_batch(self.src[split], idx, params, resize_hw,
                             self.crop_hw, self.dtype, out=out)

    def epoch_order(self, epoch: int) -> Tuple[List[int], List[int]]:
        """Sample order of one epoch, both domains: the two shuffle buffers
        share one generator and are drawn alternately, as in
        Pipeline.train_epoch."""
        g = torch.Generator().manual_seed(self.seed * 100003 + epoch)
        a = iter(ShuffleBuffer(list(range(self.num_train)), 256, g))
        b = iter(ShuffleBuffer(list(range(self.num_train)), 256, g))
        ia, ib = [], []
        for _ in range(self.num_train):
            ia.append(next(a))
            ib.append(next(b))
        return ia, ib

    def train_epoch(self, epoch: int, out=None):
        """Yields (x, y) local batches; same shuffle series on every rank.
        out=(sx, sy): full-size batches are written into these tensors and
        they are what is yielded."""
        pa, pb = (self._upload_params(self.epoch_params(epoch))
                  if self.augment == "epoch" else self._train_params)
        ia, ib = self.epoch_order(epoch)
        n = self.num_train
        order = make_idx(ia + ib, max(n, 1), self.device)  # one upload
        sx, sy = out if out is not None else (None, None)
        for s in range(self.train_steps):
            lo, hi = self._rank_range(s * self.global_batch,
                                      min((s + 1) * self.global_batch, n))
            yield (self._batch("trainA", order[lo:hi], pa, self.resize_hw, sx),
                   self._batch("trainB", order[n + lo:n + hi], pb,
                               self.resize_hw, sy))

    def test_epoch(self):
        for s in range(self.test_steps):
            lo, hi = self._rank_range(
                s * self.global_batch,
                min((s + 1) * self.global_batch, self.num_test))
            idx = self._test_idx[lo:hi]
            yield (self._batch("testA", idx, self._test_params, self.crop_hw),
                   self._batch("testB", idx, self._test_params, self.crop_hw))

    def plot_pairs(self, n: int = 5):
        for i in range(min(n, self.num_test)):
            idx = self._test_idx[i:i + 1]
            yield tuple(augment_batch(self.src[s], idx, self._test_params,
                                      self.crop_hw, self.crop_hw, self.dtype)
                        for s in ("testA", "testB"))
