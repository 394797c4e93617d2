"""The input side of a training step on the device: what data/data.py:get_dataloaders + build_transform (data.py:254-315)
do with torchvision, timm and a worker pool, for the fixed-size data sets, as one kernel launch per step.

    DeviceDataset    uint8 images [N, C, H, W] and int64 labels, resident on the device
    RaggedDeviceDataset  uint8 images of different sizes in one flat buffer, with an offset and a shape per image
    DeviceTransform  the training / evaluation transform of a config (sizes, mean / std, probabilities)
    DeviceLoader     TensorLoader's order, sharding and length; yields (x float32, y int64) device tensors

Every random decision is a function of (seed, epoch, dataset index) (ops.augment_plan), never of the batch or the rank, so N
ranks see exactly the images one rank sees.

torchvision's RandAugment(num_ops=randaug_n) after the first crop and timm's rand-m9-mstd0.5-inc1 after the second are opt-in
(`auto_augment=True`): ops.randaug_plan draws a second record per sample -- two flips and four op slots, each a PIL primitive
with its parameters -- and ops.augment_batch_ra executes it between the crops, every primitive byte for byte PIL's.  Without
the option the two policies are not applied and the two flips of the reference merge into one (from_config warns).

Image sets whose files differ in size (flowers-17 / -102) are decoded once, offline (tools/pack_images.py), and kept as a
RaggedDeviceDataset; DeviceTransform.from_config(variable_size=True) gives their transform -- RandomResizedCrop of the
sample's own H_n x W_n rectangle when training, Resize(256) of the shorter side and CenterCrop(224) for evaluation -- and
ops.augment_plan_ragged / ops.augment_batch_ragged run it.  The rectangle geometry of Resize and CenterCrop restates
torchvision's formulas by construction (torchvision is not a dependency); the pixels are pinned to PIL.
"""
import math
import warnings

import numpy as np
import torch

from . import ops

IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PLAIN_SETS = ("mnist", "fmnist", "usps")                      # data.py:270-273: ToTensor() alone, training and evaluation
VARIABLE_SIZE_SETS = ("flowers-17", "flowers-102", "reuters")  # need decoding / are not images
NOT_IMAGE_SETS = ("reuters",)
RAGGED_ALIGN = 16                                             # every image of a RaggedDeviceDataset starts on such a boundary
RAGGED_MAX_SIDE = 2048
TIMM_SCALE, TIMM_RATIO, TIMM_HFLIP = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0), 0.5   # create_transform(is_training=True) defaults


RAGGED_NO_AUTO_AUGMENT = ("the device pipeline does not apply RandAugment / auto-augment (auto_augment=True) to a variable-size "
                          "image set: the policy executor works on an S x S image resident in LDS with two spare buffers, and "
                          "224 x 224 x 3 bytes do not fit there three times")


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

    @property
    def device(self):
        return self.images.device

    @classmethod
    def from_npz(cls, path, device="cuda", images="images", labels="labels"):
        """A local .npz with an `images` (uint8) and a `labels` array."""
        with np.load(path) as z:
            return cls(torch.from_numpy(z[images]), torch.from_numpy(z[labels].astype(np.int64)), device)


def pack_ragged(images, layout=None):
    """uint8 images of different sizes -> (data uint8 [bytes], offsets int64 [N], shapes int32 [N, 2], C): each image planar
    [C][H][W] at a multiple of RAGGED_ALIGN.  An image is [H, W], [H, W, C] or [C, H, W]; `layout` ("HWC" / "CHW") settles a
    three-dimensional one, otherwise a last dimension of 1 or 3 means [H, W, C]."""
    planes, C = [], None
    for n, im in enumerate(images):
        im = np.asarray(im)
        if im.dtype != np.uint8:
            raise ValueError(f"pack_ragged: image {n} must be uint8, got {im.dtype}")
        if im.ndim == 2:
            im = im[None]
        elif im.ndim == 3 and (layout == "HWC" or (layout is None and im.shape[2] in (1, 3))):
            im = im.transpose(2, 0, 1)
        if im.ndim != 3 or im.shape[0] not in (1, 3):
            raise ValueError(f"pack_ragged: image {n}: expected [H, W], [H, W, C] or [C, H, W] with 1 or 3 channels, got {im.shape}")
        if C is None:
            C = im.shape[0]
        if im.shape[0] != C:
            raise ValueError(f"pack_ragged: image {n} has {im.shape[0]} channels, the set has {C}")
        planes.append(np.ascontiguousarray(im))
    if not planes:
        raise ValueError("pack_ragged: no image")
    shapes = np.array([p.shape[1:] for p in planes], np.int32).reshape(-1, 2)
    sizes = C * shapes[:, 0].astype(np.int64) * shapes[:, 1]
    padded = (sizes + RAGGED_ALIGN - 1) // RAGGED_ALIGN * RAGGED_ALIGN
    offsets = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    data = np.zeros(int(padded.sum()), np.uint8)
    for p, o, k in zip(planes, offsets, sizes):
        data[o:o + k] = p.reshape(-1)
    return data, offsets, shapes, C


class RaggedDeviceDataset:
    """uint8 images of different sizes, moved to `device` once: `data` one flat buffer (image n planar [C][H_n][W_n] at
    offsets[n], a multiple of 16), `offsets` int64 [N], `shapes` int32 [N, 2] = (H_n, W_n), `labels` int64 [N]; C (1 or 3) is
    one value for the whole set, max_h and max_w bound every side."""

    def __init__(self, data, offsets, shapes, labels, channels, device="cuda"):
        data, offsets = torch.as_tensor(data), torch.as_tensor(offsets).to(torch.int64).reshape(-1)
        shapes, labels = torch.as_tensor(shapes).to(torch.int32), torch.as_tensor(labels)
        C = int(channels)
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError(f"RaggedDeviceDataset: data must be a flat uint8 buffer, got {data.dtype} {tuple(data.shape)}")
        if C not in (1, 3):
            raise ValueError(f"RaggedDeviceDataset: {C} channels (1 or 3)")
        N = offsets.numel()
        if N == 0 or tuple(shapes.shape) != (N, 2):
            raise ValueError(f"RaggedDeviceDataset: shapes must be [N, 2] for the N = {N} offsets, got {tuple(shapes.shape)}")
        if labels.shape[0] != N:
            raise ValueError(f"RaggedDeviceDataset: one label per image ({labels.shape[0]} labels, {N} images)")
        if int(shapes.min()) < 1:
            raise ValueError("RaggedDeviceDataset: every side must be at least 1")
        if int(shapes.max()) > RAGGED_MAX_SIDE:
            raise ValueError(f"RaggedDeviceDataset: a side of {int(shapes.max())} pixels (at most {RAGGED_MAX_SIDE})")
        if bool((offsets % RAGGED_ALIGN != 0).any()) or int(offsets[0]) < 0:
            raise ValueError(f"RaggedDeviceDataset: offsets must be non-negative multiples of {RAGGED_ALIGN}")
        if N > 1 and bool((offsets[1:] <= offsets[:-1]).any()):
            raise ValueError("RaggedDeviceDataset: offsets must be increasing")
        ends = offsets + C * shapes[:, 0].to(torch.int64) * shapes[:, 1].to(torch.int64)
        if bool((ends > data.numel()).any()):
            n = int((ends > data.numel()).nonzero()[0])
            raise ValueError(f"RaggedDeviceDataset: image {n} ends past the data buffer ({int(ends[n])} > {data.numel()} bytes)")
        self.C, self.max_h, self.max_w = C, int(shapes[:, 0].max()), int(shapes[:, 1].max())
        self.data, self.offsets = data.contiguous().to(device), offsets.contiguous().to(device)
        self.shapes = shapes.contiguous().to(device)
        self.labels = labels.reshape(N, -1)[:, 0].to(torch.int64).contiguous().to(device)

    def __len__(self):
        return self.offsets.numel()

    @property
    def device(self):
        return self.data.device

    def image(self, n):
        """Image n as a [C, H_n, W_n] view of the buffer."""
        h, w = (int(v) for v in self.shapes[n])
        o = int(self.offsets[n])
        return self.data[o:o + self.C * h * w].view(self.C, h, w)

    @classmethod
    def from_arrays(cls, images, labels, device="cuda", layout=None):
        """A list of uint8 images, each [H, W], [H, W, C] or [C, H, W] (see pack_ragged), and one label each."""
        data, offsets, shapes, C = pack_ragged(images, layout)
        return cls(torch.from_numpy(data), torch.from_numpy(offsets), torch.from_numpy(shapes), torch.as_tensor(np.asarray(labels)), C, device)

    @classmethod
    def from_npz(cls, path, device="cuda", prefix=""):
        """A local .npz as tools/pack_images.py writes it: data, offsets, shapes, labels, channels (prefix "test_": the held-out
        part)."""
        with np.load(path) as z:
            return cls(torch.from_numpy(z[prefix + "data"]), torch.from_numpy(z[prefix + "offsets"].astype(np.int64)),
                       torch.from_numpy(z[prefix + "shapes"].astype(np.int32)), torch.from_numpy(z[prefix + "labels"].astype(np.int64)),
                       int(z["channels"]), device)

    def to_npz_arrays(self, prefix=""):
        """The arrays from_npz reads, on the host."""
        return {prefix + "data": self.data.cpu().numpy(), prefix + "offsets": self.offsets.cpu().numpy(),
                prefix + "shapes": self.shapes.cpu().numpy(), prefix + "labels": self.labels.cpu().numpy(),
                "channels": np.int64(self.C)}


class DeviceTransform:
    """build_transform (data.py:254-315) as numbers: what ops.augment_plan / ops.augment_batch need."""

    def __init__(self, train, num_channels, input_size, mean, std, plain=False, scale=(0.08, 1.0), ratio=(0.75, 1.3333),
                 two_stage=True, flip_p=0.5, erase_p=0.25, auto_augment=False, randaug_n=0, autoaugment=False, flip1_p=0.5,
                 variable_size=False):
        self.train, self.C, self.S, self.plain = bool(train), int(num_channels), int(input_size), bool(plain)
        # variable_size: the transform of a RaggedDeviceDataset; the centre window's offsets then depend on the sample's
        # shape and are computed by the kernel (off is None for the evaluation transform)
        self.variable_size = bool(variable_size)
        if self.variable_size and auto_augment:
            raise NotImplementedError(RAGGED_NO_AUTO_AUGMENT)
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
            self.off = None if self.variable_size else int(round((self.R - self.S) / 2.0))
        self._dev = {}

    @classmethod
    def from_config(cls, config, train, strict=False, auto_augment=False, variable_size=False):
        """`variable_size`: the transform for a RaggedDeviceDataset, for any image set (the flowers sets included)."""
        d = config["data"]
        name, S, C = d["dataset"], int(d["input_size"]), int(d["num_channels"])
        if variable_size:
            if name in NOT_IMAGE_SETS:
                raise ValueError(f"DeviceTransform: data set '{name}' is not an image set")
            if auto_augment:
                raise NotImplementedError(RAGGED_NO_AUTO_AUGMENT)
        elif name in VARIABLE_SIZE_SETS:
            raise ValueError(f"DeviceTransform: data set '{name}' is not a fixed-size image set (it needs decoding and a resize "
                             "per file); the device pipeline covers the sets that fit in memory as uint8 [N, C, H, H]")
        if name in PLAIN_SETS:
            # level / 255 alone.  The kernel still runs its two resize passes, H -> H: every coefficient row is a single 1,
            # so the bytes pass through unchanged; a copy-only path would save a few microseconds per batch of 28 x 28 images.
            return cls(train, C, S, (0.0,) * C, (1.0,) * C, plain=True, variable_size=variable_size)
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
                   randaug_n=int(a.get("randaug_n", 2)), autoaugment=bool(a.get("autoaugment", True)), flip1_p=p1,
                   variable_size=variable_size)

    def stats(self, device):
        """(mean, std) as float32 tensors on `device`."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.tensor(self.mean, dtype=torch.float32, device=device),
                              torch.tensor(self.std, dtype=torch.float32, device=device))
        return self._dev[key]

    def apply(self, dataset, index, out, params, seed, epoch, out_u8=None, ra=None, scratch=None):
        """out[:len(index)] <- the transformed rows `index` (int64, on the device) of `dataset`; two launches when training
        with augmentation (three with auto_augment, which also needs the record buffer `ra`), one otherwise.  A
        RaggedDeviceDataset takes three launches when training (plan, crop 1 into `scratch`, crop 2 and the output stage)."""
        if isinstance(dataset, RaggedDeviceDataset):
            return self._apply_ragged(dataset, index, out, params, seed, epoch, out_u8, scratch)
        if self.variable_size:
            raise ValueError("DeviceTransform: a variable_size transform needs a RaggedDeviceDataset")
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


    def _apply_ragged(self, ds, index, out, params, seed, epoch, out_u8, scratch):
        if self.auto_augment:
            raise NotImplementedError(RAGGED_NO_AUTO_AUGMENT)
        if not self.variable_size:
            raise ValueError("DeviceTransform: a RaggedDeviceDataset needs from_config(variable_size=True)")
        if ds.C != self.C:
            raise ValueError(f"DeviceTransform: {ds.C}-channel data, {self.C}-channel transform")
        mean, std = self.stats(ds.device)
        if not self.train:
            return ops.augment_batch_ragged(ds.data, ds.offsets, ds.shapes, ds.C, ds.max_h, ds.max_w, index, None, out, self.S, self.R,
                                            mean, std, seed, epoch, out_u8=out_u8)
        if scratch is None:
            raise ValueError("DeviceTransform.apply: training on a RaggedDeviceDataset needs the `scratch` buffer "
                             "(uint8, ops.augment_ragged_scratch_bytes(B, C, S))")
        if self.augment:
            ops.augment_plan_ragged(index, ds.shapes, params, self.S, self.scale, (math.log(self.ratio[0]), math.log(self.ratio[1])),
                                    TIMM_SCALE if self.two_stage else None, (math.log(TIMM_RATIO[0]), math.log(TIMM_RATIO[1])),
                                    self.flip_p, self.erase_p, seed, epoch)
        else:                                                  # plain sets: the whole image -> S x S, no flip, no erase
            params.zero_()
            params[:index.numel(), 2:4] = ds.shapes[index]
        return ops.augment_batch_ragged(ds.data, ds.offsets, ds.shapes, ds.C, ds.max_h, ds.max_w, index, params, out, self.S, self.S,
                                        mean, std, seed, epoch, scratch=scratch, out_u8=out_u8)


class DeviceLoader:
    """train.TensorLoader over a DeviceDataset or a RaggedDeviceDataset: the same index order, rank interleave and len() for the same arguments, so
    that switching loaders changes the pixels and nothing else.  Yields (x [b, C, S, S] float32, y [b] int64) on the device.

    Lifetime of a batch: x is a VIEW of one of two pre-allocated buffers and is overwritten when the batch after the next
    one is produced; use it in the step it was yielded for, or clone() it to keep it.  y is a tensor of its own (b * 8
    bytes) and may be kept, as evaluate_kmeans and visualize_umap_progression do."""

    def __init__(self, dataset, batch_size, transform, shuffle=False, rank=0, world_size=1, seed=0, drop_last=False):
        self.dataset, self.batch_size, self.transform, self.shuffle = dataset, int(batch_size), transform, shuffle
        self.rank, self.world, self.seed, self.drop_last, self.epoch = rank, world_size, seed, drop_last, 0
        self._ring, self._slot, self._scratch = None, 0, None
        if isinstance(dataset, RaggedDeviceDataset) and getattr(transform, "auto_augment", False):
            raise NotImplementedError(RAGGED_NO_AUTO_AUGMENT)

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
            t, dev, B = self.transform, self.dataset.device, self.batch_size
            # one scratch for both slots: stream order finishes a batch's second crop before the next batch's first
            self._scratch = (torch.empty(ops.augment_ragged_scratch_bytes(B, t.C, t.S), dtype=torch.uint8, device=dev)
                             if isinstance(self.dataset, RaggedDeviceDataset) and t.train else None)
            self._ring = [(torch.empty(B, t.C, t.S, t.S, dtype=torch.float32, device=dev),
                           torch.zeros(B, ops.AUGMENT_PARAMS, dtype=torch.int32, device=dev),
                           torch.zeros(B, ops.RANDAUG_PARAMS, dtype=torch.int32, device=dev) if t.auto_augment else None)
                          for _ in range(2)]
        return self._ring

    def __iter__(self):
        epoch = self.epoch
        idx = self.epoch_indices().to(self.dataset.device)              # one copy per epoch; batches are views of it
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
            self.transform.apply(self.dataset, j, x, params, self.seed, epoch, ra=ra, scratch=self._scratch)
            # the labels are not ring views: consumers collect them over a whole loader (evaluation.py)
            yield x[:b], self.dataset.labels[j]
