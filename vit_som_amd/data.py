"""The input side of a training step on the device: what data/data.py:get_dataloaders + build_transform (data.py:254-315)
do with torchvision, timm and a worker pool, for the fixed-size data sets, as one kernel launch per step.

    DeviceDataset    uint8 images [N, C, H, W] and int64 labels, resident on the device
    DeviceTransform  the training / evaluation transform of a config (sizes, mean / std, probabilities)
    DeviceLoader     TensorLoader's order, sharding and length; yields (x float32, y int64) device tensors

Every random decision is a function of (seed, epoch, dataset index) (ops.augment_plan), never of the batch or the rank, so N
ranks see exactly the images one rank sees.

torchvision's RandAugment(num_ops=randaug_n) after the first crop and timm's rand-m9-mstd0.5-inc1 after the second are opt-in
(`auto_augment=True`): ops.randaug_plan draws a second record per sample -- two flips and four op slots, each a PIL primitive
with its parameters -- and ops.augment_batch_ra executes it between the crops, every primitive byte for byte PIL's.  Without
the option the two policies are not applied and the two flips of the reference merge into one (from_config warns).
"""
import math
import warnings

import numpy as np
import torch

from . import ops

IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PLAIN_SETS = ("mnist", "fmnist", "usps")                      # data.py:270-273: ToTensor() alone, training and evaluation
VARIABLE_SIZE_SETS = ("flowers-17", "flowers-102", "reuters")  # need decoding / are not images
TIMM_SCALE, TIMM_RATIO, TIMM_HFLIP = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0), 0.5   # create_transform(is_training=True) defaults


class DeviceDataset:
    """uint8 images [N, C, H, W] ([N, H, W, C] and [N, H, W] are permuted once) and int64 labels, moved to `device` once."""

    def __init__(self, images_u8, labels, device="cuda"):
        images_u8, labels = torch.as_tensor(images_u8), torch.as_tensor(labels)
        if images_u8.dtype != torch.uint8:
            raise ValueError(f"DeviceDataset: images must be uint8, got {images_u8.dtype}")
        if images_u8.dim() == 3:
            images_u8 = images_u8[:, None]
        elif images_u8.dim() == 4 and images_u8.shape[1] not in (1, 3) and images_u8.shape[3] in (1, 3):
            images_u8 = images_u8.permute(0, 3, 1, 2)
        if images_u8.dim() != 4 or images_u8.shape[1] not in (1, 3) or images_u8.shape[2] != images_u8.shape[3]:
            raise ValueError(f"DeviceDataset: expected [N, C, H, H] with 1 or 3 channels, got {tuple(images_u8.shape)}")
        if labels.shape[0] != images_u8.shape[0]:
            raise ValueError("DeviceDataset: one label per image")
        self.images = images_u8.contiguous().to(device)
        self.labels = labels.reshape(labels.shape[0], -1)[:, 0].to(torch.int64).contiguous().to(device)

    def __len__(self):
        return self.images.shape[0]

    @classmethod
    def from_npz(cls, path, device="cuda", images="images", labels="labels"):
        """A local .npz with an `images` (uint8) and a `labels` array."""
        with np.load(path) as z:
            return cls(torch.from_numpy(z[images]), torch.from_numpy(z[labels].astype(np.int64)), device)


class DeviceTransform:
    """build_transform (data.py:254-315) as numbers: what ops.augment_plan / ops.augment_batch need."""

    def __init__(self, train, num_channels, input_size, mean, std, plain=False, scale=(0.08, 1.0), ratio=(0.75, 1.3333),
                 two_stage=True, flip_p=0.5, erase_p=0.25, auto_augment=False, randaug_n=0, autoaugment=False, flip1_p=0.5):
        self.train, self.C, self.S, self.plain = bool(train), int(num_channels), int(input_size), bool(plain)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        self.augment = self.train and not self.plain
        self.scale, self.ratio = tuple(float(v) for v in scale), tuple(float(v) for v in ratio)
        self.two_stage, self.flip_p, self.erase_p = bool(two_stage), float(flip_p), float(erase_p)
        # auto_augment: RandAugment (randaug_n slots, NEAREST, fill 0) and timm's rand-m9 (autoaugment: two slots, BICUBIC,
        # fill = timm's img_mean) through ops.randaug_plan / ops.augment_batch_ra; flip1_p: the reference's own flip
        self.auto_augment = bool(auto_augment) and self.train and not self.plain
        self.randaug_n, self.autoaugment, self.flip1_p = int(randaug_n), bool(autoaugment), float(flip1_p)
        if self.auto_augment and not 0 <= self.randaug_n <= 2:
            raise ValueError(f"DeviceTransform: randaug_n = {self.randaug_n} (the record holds 0 to 2 torchvision slots)")
        self.fill_tv = (0,) * self.C
        self.fill_timm = tuple(min(255, round(255 * m)) for m in self.mean)
        if self.train or self.plain:
            self.R, self.off = self.S, 0
        else:                                                  # Resize(int(S / crop_pct)) + CenterCrop(S), data.py:306-310
            crop_pct = 0.875 if self.S <= 224 else 1.0
            self.R = int(self.S / crop_pct)
            self.off = int(round((self.R - self.S) / 2.0))
        self._dev = {}

    @classmethod
    def from_config(cls, config, train, strict=False, auto_augment=False):
        d = config["data"]
        name, S, C = d["dataset"], int(d["input_size"]), int(d["num_channels"])
        if name in VARIABLE_SIZE_SETS:
            raise ValueError(f"DeviceTransform: data set '{name}' is not a fixed-size image set (it needs decoding and a resize "
                             "per file); the device pipeline covers the sets that fit in memory as uint8 [N, C, H, H]")
        if name in PLAIN_SETS:
            # level / 255 alone.  The kernel still runs its two resize passes, H -> H: every coefficient row is a single 1,
            # so the bytes pass through unchanged; a copy-only path would save a few microseconds per batch of 28 x 28 images.
            return cls(train, C, S, (0.0,) * C, (1.0,) * C, plain=True)
        if C == 1:
            mean, std = (0.5,), (0.5,)
        elif name in ("cifar-10", "cifar-100"):
            mean, std = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
        elif name == "medmnist":
            mean, std = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
        else:
            mean, std = IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
        a = d.get("augment") or {}
        if train:
            if a.get("remode", "pixel") != "pixel":
                raise ValueError(f"DeviceTransform: remode '{a.get('remode')}' (only 'pixel' is implemented)")
            if int(a.get("recount", 1)) > 1:
                raise ValueError("DeviceTransform: recount > 1 (one erase box per image is implemented)")
            if not auto_augment and (int(a.get("randaug_n", 2)) > 0 or a.get("autoaugment", True)):
                by_default = [k for k in ("randaug_n", "autoaugment") if k not in a]
                msg = ("DeviceTransform: RandAugment / auto-augment (randaug_n, autoaugment) are not applied by the device "
                       "pipeline: crops, flip and random erasing only")
                if by_default:                                 # get_dataloaders' own defaults: randaug_n=2, autoaugment on
                    msg += f" ({', '.join(by_default)} not in the config: the reference's defaults turn them on)"
                if strict:
                    raise NotImplementedError(msg)
                warnings.warn(msg, stacklevel=2)
        p1 = float(a.get("horizontal_flip", 0.5))
        # RandomHorizontalFlip(p1) then timm's own flip (0.5): one flip with the probability that exactly one happens
        flip_p = p1 * (1.0 - TIMM_HFLIP) + TIMM_HFLIP * (1.0 - p1)
        return cls(train, C, S, mean, std, scale=a.get("resize_scale", (0.08, 1.0)), ratio=a.get("resize_ratio", (0.75, 1.3333)),
                   two_stage=True, flip_p=flip_p, erase_p=float(a.get("reprob", 0.25)), auto_augment=auto_augment,
                   randaug_n=int(a.get("randaug_n", 2)), autoaugment=bool(a.get("autoaugment", True)), flip1_p=p1)

    def stats(self, device):
        """(mean, std) as float32 tensors on `device`."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.tensor(self.mean, dtype=torch.float32, device=device),
                              torch.tensor(self.std, dtype=torch.float32, device=device))
        return self._dev[key]

    def apply(self, dataset, index, out, params, seed, epoch, out_u8=None, ra=None):
        """out[:len(index)] <- the transformed rows `index` (int64, on the device) of `dataset`; two launches when training
        with augmentation (three with auto_augment, which also needs the record buffer `ra`), one otherwise."""
        src = dataset.images
        if src.shape[1] != self.C:
            raise ValueError(f"DeviceTransform: {src.shape[1]}-channel data, {self.C}-channel transform")
        mean, std = self.stats(src.device)
        if self.augment:
            ops.augment_plan(index, params, src.shape[0], src.shape[2], self.S, self.scale, (math.log(self.ratio[0]), math.log(self.ratio[1])),
                             TIMM_SCALE if self.two_stage else None, (math.log(TIMM_RATIO[0]), math.log(TIMM_RATIO[1])),
                             self.flip_p, self.erase_p, seed, epoch)
        if self.auto_augment:
            if ra is None:
                raise ValueError("DeviceTransform.apply: auto_augment needs the record buffer `ra` [B, ops.RANDAUG_PARAMS] int32")
            ops.randaug_plan(index, ra, src.shape[0], self.S, self.randaug_n, self.autoaugment, self.flip1_p, self.fill_tv,
                             self.fill_timm, seed, epoch)
            return ops.augment_batch_ra(src, index, params, ra, out, self.S, mean, std, seed, epoch, out_u8=out_u8)
        return ops.augment_batch(src, index, params if self.augment else None, out, self.S, self.R, self.off, mean, std, seed, epoch,
                                 out_u8=out_u8)


class DeviceLoader:
    """train.TensorLoader over a DeviceDataset: the same index order, rank interleave and len() for the same arguments, so
    that switching loaders changes the pixels and nothing else.  Yields (x [b, C, S, S] float32, y [b] int64) on the device.

    Lifetime of a batch: x is a VIEW of one of two pre-allocated buffers and is overwritten when the batch after the next
    one is produced; use it in the step it was yielded for, or clone() it to keep it.  y is a tensor of its own (b * 8
    bytes) and may be kept, as evaluate_kmeans and visualize_umap_progression do."""

    def __init__(self, dataset, batch_size, transform, shuffle=False, rank=0, world_size=1, seed=0, drop_last=False):
        self.dataset, self.batch_size, self.transform, self.shuffle = dataset, int(batch_size), transform, shuffle
        self.rank, self.world, self.seed, self.drop_last, self.epoch = rank, world_size, seed, drop_last, 0
        self._ring, self._slot = None, 0

    def __len__(self):
        n = len(self.dataset) // self.world
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def epoch_indices(self):
        """This rank's dataset rows for the current epoch, in order (CPU int64); advances the epoch like TensorLoader."""
        n = len(self.dataset)
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + self.epoch)) if self.shuffle else torch.arange(n)
        self.epoch += 1
        return idx[: (n // self.world) * self.world][self.rank::self.world]

    def index_batches(self):
        """The batches of one epoch as CPU index tensors (no device work)."""
        idx = self.epoch_indices()
        for i in range(0, len(idx), self.batch_size):
            j = idx[i:i + self.batch_size]
            if self.drop_last and len(j) < self.batch_size:
                break
            yield j

    def _buffers(self):
        if self._ring is None:
            t, dev, B = self.transform, self.dataset.images.device, self.batch_size
            self._ring = [(torch.empty(B, t.C, t.S, t.S, dtype=torch.float32, device=dev),
                           torch.zeros(B, ops.AUGMENT_PARAMS, dtype=torch.int32, device=dev),
                           torch.zeros(B, ops.RANDAUG_PARAMS, dtype=torch.int32, device=dev) if t.auto_augment else None)
                          for _ in range(2)]
        return self._ring

    def __iter__(self):
        epoch = self.epoch
        idx = self.epoch_indices().to(self.dataset.images.device)       # one copy per epoch; batches are views of it
        ring = self._buffers()
        for i in range(0, len(idx), self.batch_size):
            j = idx[i:i + self.batch_size]
            b = j.numel()
            if self.drop_last and b < self.batch_size:
                break
            # A ring of two pre-allocated batches: the batch handed out last time stays intact while this one is written.
            # Nothing waits: the kernels go to the stream the consumer's step is queued on, so this launch runs after every
            # earlier reader of the slot it overwrites (the step before last) -- stream order alone guarantees it.
            x, params, ra = ring[self._slot]
            self._slot ^= 1
            self.transform.apply(self.dataset, j, x, params, self.seed, epoch, ra=ra)
            # the labels are not ring views: consumers collect them over a whole loader (evaluation.py)
            yield x[:b], self.dataset.labels[j]
