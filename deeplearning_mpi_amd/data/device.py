"""Device-resident input pipeline.

The reference feeds its GPUs through ``torch.utils.data.DataLoader`` worker processes: per-sample
Python/PIL transforms, collation, pinned host buffers and a host->device copy every step
(/root/reference/pytorch/resnet/main.py:82-97, unet/train.py:78-101).  Its datasets are small
(CIFAR-10: 150 MB of uint8; the UNet cell images at scale 0.2: ~0.3 GB as fp32) next to 288 GB of
HBM3E per MI355X, so here the dataset is made resident on the GPU once and every batch is one
device-side gather:

* :class:`DeviceImageDataset` -- uint8 HWC images + labels in HBM; a batch is ONE HIP kernel
  (``csrc/kernels/data.hip``): gather by index + RandomCrop(32, padding=4) + RandomHorizontalFlip
  + ToTensor + Normalize (the reference CIFAR transform), written as fp32 NCHW.  The augmentation
  parameters are a hash of (seed, epoch, dataset index), so they do not depend on the batch size,
  rank count or worker count, and :func:`image_batch_reference` reproduces them exactly on the CPU.
  With ``mix=MixConfig(...)`` the same kernel also mixes the batch with itself (mixup / CutMix,
  ``data/mix.py``): "augment as today, then mix", and it writes ``labels_b`` and the device ``lam``.
  With ``rrc=RrcConfig(...)`` or ``eval_crop=`` the batch is resampled to ``out_size`` instead
  (RandomResizedCrop + flip, or resize + centre crop; ``data/rrc.py``, ``csrc/kernels/rrc.hip``), still ONE
  kernel, through the sample's row of the epoch's crop table.
* :class:`DeviceCachedDataset` -- any deterministic map-style dataset (the reference UNet's
  image/mask dataset has no random augmentation) materialised once on the device; batches are
  ``index_select`` gathers.
* :class:`DeviceSegDataset` -- the same image / mask pairs with geometric augmentation (flip, scale, rotate,
  translate, crop; ``data/seg_aug.py``): a batch is ONE HIP kernel (``csrc/kernels/seg_aug.hip``) that gathers
  and resamples image and mask through the sample's row of the epoch's parameter table.
* :class:`DeviceBatches` -- iterates any of them in :class:`DistributedSampler` order (the epoch's index
  list goes to the device in one copy), optionally writing into fixed tensors so a captured
  hipGraph step can consume them without a copy.
"""
from __future__ import annotations

import os
import warnings

import numpy as np
import torch

from .datasets import CIFAR10, CIFAR_MEAN, CIFAR_STD
from .mix import KINDS, MixConfig, draw_mix, mix_reference
from .rrc import RrcConfig, center_box, draw_rrc, rrc_reference
from .seg_aug import SegAugConfig, draw_seg_aug, seg_aug_reference

_M32 = 0xFFFFFFFF


def _fmix32(h: torch.Tensor) -> torch.Tensor:
    """murmur3 finalizer on uint32 values held in int64 (mod 2^32 arithmetic), = data.hip:fmix32."""
    h = h & _M32
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def _aug_params(idx: torch.Tensor, seed: int, epoch: int, pad: int):
    """(crop row offset, crop col offset, flip) per sample, exactly as the HIP kernel draws them."""
    base = ((seed * 0x9E3779B1) + (epoch * 0x85EBCA77)) & _M32
    h = _fmix32((idx.to(torch.int64) & _M32) + base)
    span = 2 * pad + 1
    return h % span, (h >> 8) % span, (h >> 16) & 1


def image_batch_reference(data_hwc_u8: torch.Tensor, labels: torch.Tensor, idx: torch.Tensor, pad: int,
                          augment: bool, seed: int, epoch: int, mean, std):
    """CPU/torch reference of the device batch kernel (also the CPU execution path)."""
    idx = idx.to(torch.int64).cpu()
    imgs = data_hwc_u8[idx.to(data_hwc_u8.device)].cpu().permute(0, 3, 1, 2).float() / 255.0   # [B, C, H, W]
    B, C, H, W = imgs.shape
    if augment:
        oi, oj, flip = _aug_params(idx, seed, epoch, pad)
        padded = torch.nn.functional.pad(imgs, (pad, pad, pad, pad))
        out = torch.empty_like(imgs)
        for b in range(B):
            crop = padded[b, :, int(oi[b]):int(oi[b]) + H, int(oj[b]):int(oj[b]) + W]
            out[b] = crop.flip(-1) if int(flip[b]) else crop
        imgs = out
    m = torch.tensor(mean[:C], dtype=torch.float32).view(1, C, 1, 1)
    s = torch.tensor(std[:C], dtype=torch.float32).view(1, C, 1, 1)
    return (imgs - m) / s, labels.cpu()[idx]


class DeviceImageDataset:
    """uint8 images [N, H, W, C] + int64 labels resident on ``device``; ``batch`` assembles
    normalised (optionally crop/flip-augmented) fp32 NCHW batches with one kernel.

    ``rrc`` (training: RandomResizedCrop + flip) or ``eval_crop`` (evaluation: the centred square of that fraction
    of the shorter side) switch to the resampling kernel: batches are ``[B, C, *out_size]`` (default: the stored
    size), cropped through the epoch's table (``data/rrc.py``), which is drawn on the host and copied to the device
    when the epoch changes -- one small copy per epoch, none per step.  ``augment`` / ``pad`` then play no part,
    and a mix is applied to the finished batch (``mix_batch_``), not here.  On a CPU device ``batch`` runs
    :func:`rrc_reference`."""

    def __init__(self, images_hwc_u8, labels, device, augment=False, pad=4, mean=CIFAR_MEAN, std=CIFAR_STD, seed=0,
                 mix: MixConfig = None, rrc: RrcConfig = None, out_size=None, eval_crop=None):
        self.device = torch.device(device)
        self.data = torch.as_tensor(np.ascontiguousarray(images_hwc_u8)).to(self.device)
        self.labels = torch.as_tensor(np.asarray(labels, dtype=np.int64)).to(self.device)
        assert self.data.dtype == torch.uint8 and self.data.dim() == 4 and self.data.shape[-1] <= 3
        self.N, self.H, self.W, self.C = self.data.shape
        self.augment, self.pad, self.seed = augment, pad, seed
        self.mean, self.std = list(mean)[:self.C], list(std)[:self.C]
        self.mix = mix
        self.rrc, self.eval_crop = rrc, eval_crop
        self.resample = rrc is not None or eval_crop is not None
        if self.resample:
            if rrc is not None and eval_crop is not None:
                raise ValueError("rrc (training) and eval_crop (evaluation) exclude each other")
            if rrc is not None and not isinstance(rrc, RrcConfig):
                raise TypeError("rrc must be an RrcConfig")
            if mix is not None:
                raise ValueError("a resampled batch is mixed after the batch kernel (mix_batch_), not by mix=")
            if self.C not in (1, 3) or self.labels.shape != (self.N,):
                raise ValueError("the resampling kernel takes 1 or 3 channels and one label per image")
            size = (self.H, self.W) if out_size is None else out_size
            self.Ho, self.Wo = (int(size), int(size)) if np.ndim(size) == 0 else (int(size[0]), int(size[1]))
            if self.Ho < 1 or self.Wo < 1:
                raise ValueError(f"out_size must be at least (1, 1), got {out_size}")
            if eval_crop is not None:
                self._fixed_box = center_box(self.H, self.W, float(eval_crop))
            self.redraws = 0                 # tables drawn (and copied to the device) so far
            self._epoch = self._table = self._table_np = None
        elif out_size is not None:
            raise ValueError("out_size needs rrc or eval_crop: the crop/flip pipeline keeps the stored size")
        self._native = None
        if self.device.type == "cuda":
            from .._ext import native

            self._native = native()

    @classmethod
    def cifar10(cls, root, train, device, augment=None, seed=0, mix=None, mean=CIFAR_MEAN, std=CIFAR_STD):
        data, targets = CIFAR10._load(root, train)
        return cls(data, targets, device, augment=train if augment is None else augment, mean=mean, std=std,
                   seed=seed, mix=mix)

    @classmethod
    def from_npy(cls, root, split, device, **kwargs):
        """``{root}/{split}_images.npy`` (uint8 [N, H, W, C]) and ``{split}_labels.npy`` (int64 [N]), as
        ``scripts/make_image_arrays.py`` writes them; memory-mapped, so the host never holds a second copy."""
        images = np.load(os.path.join(root, f"{split}_images.npy"), mmap_mode="r")
        labels = np.load(os.path.join(root, f"{split}_labels.npy"), mmap_mode="r")
        if images.dtype != np.uint8 or images.ndim != 4 or labels.shape != (images.shape[0],):
            raise ValueError(f"{split}: images must be uint8 [N, H, W, C] with one label each, got {images.dtype} "
                             f"{images.shape} and labels {labels.shape}")
        with warnings.catch_warnings():   # torch warns that the map is read-only; the dataset never writes to it
            warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
            return cls(images, labels, device, **kwargs)

    def table(self, epoch: int) -> torch.Tensor:
        """The crop table of ``epoch`` on the device, int32 [N, 5]; redrawn when the epoch changes (``rrc``), or the
        one centre box for every sample and epoch (``eval_crop``)."""
        if self._table is None or (self.rrc is not None and self._epoch != int(epoch)):
            if self.rrc is not None:
                self._table_np = draw_rrc(self.rrc, self.seed, int(epoch), self.N, self.H, self.W)
            else:
                self._table_np = np.ascontiguousarray(np.tile(np.array(self._fixed_box, dtype=np.int32), (self.N, 1)))
            self._table = torch.from_numpy(self._table_np).to(self.device)
            self._epoch = int(epoch)
            self.redraws += 1
        return self._table

    def __len__(self):
        return self.N

    def batch(self, idx: torch.Tensor, epoch: int = 0, out=None, batch_no: int = 0, rank: int = 0):
        """idx: int64 dataset indices on the device -> (x [B, C, H, W] fp32, y [B] int64); with ``mix`` set ->
        (x, labels_a, labels_b [B] int64, lam [1] fp32), mixed as ``draw_mix(mix, seed, epoch, rank, batch_no)``
        says."""
        B = idx.numel()
        if self.resample:
            return self._resampled_batch(idx, epoch, out)
        if self.mix is not None:
            return self._mixed_batch(idx, epoch, out, batch_no, rank)
        if out is None:
            x = torch.empty(B, self.C, self.H, self.W, dtype=torch.float32, device=self.device)
            y = torch.empty(B, dtype=torch.int64, device=self.device)
        else:
            x, y = out
        if self._native is not None:
            self._native.image_batch(self.data, self.labels, idx, self.H, self.W, self.C, self.pad, self.augment,
                                     self.seed, epoch, self.mean, self.std, x, y)
        else:
            xr, yr = image_batch_reference(self.data, self.labels, idx, self.pad, self.augment, self.seed, epoch,
                                           self.mean, self.std)
            x.copy_(xr)
            y.copy_(yr)
        return x, y

    def _resampled_batch(self, idx, epoch, out):
        B = idx.numel()
        if out is None:
            x = torch.empty(B, self.C, self.Ho, self.Wo, dtype=torch.float32, device=self.device)
            y = torch.empty(B, dtype=torch.int64, device=self.device)
        else:
            x, y = out[:2]   # (the fixed tensors of a mixed step carry labels_b and lam behind these two)
            if tuple(x.shape) != (B, self.C, self.Ho, self.Wo) or tuple(y.shape) != (B,):
                raise ValueError(f"out must be ([{B}, {self.C}, {self.Ho}, {self.Wo}], [{B}]), got {tuple(x.shape)} "
                                 f"and {tuple(y.shape)}")
        table = self.table(epoch)
        if self._native is not None:
            self._native.image_rrc_batch(self.data, self.labels, idx, table, self.mean, self.std, x, y)
        else:
            xr, yr = rrc_reference(self.data, self.labels, idx, self._table_np, self.Ho, self.Wo, self.mean, self.std)
            x.copy_(xr)
            y.copy_(yr)
        return x, y

    def _mixed_batch(self, idx, epoch, out, batch_no, rank):
        B = idx.numel()
        if out is None:
            x = torch.empty(B, self.C, self.H, self.W, dtype=torch.float32, device=self.device)
            ya = torch.empty(B, dtype=torch.int64, device=self.device)
            yb, lam = torch.empty_like(ya), torch.empty(1, dtype=torch.float32, device=self.device)
        else:
            x, ya, yb, lam = out
        p = draw_mix(self.mix, self.seed, epoch, rank, batch_no, self.H, self.W)
        if self._native is not None:
            self._native.image_batch_mix(self.data, self.labels, idx, self.H, self.W, self.C, self.pad, self.augment,
                                         self.seed, epoch, self.mean, self.std, KINDS.index(p.kind), float(p.lam),
                                         *p.box, x, ya, yb, lam)
        else:
            xr, yr = image_batch_reference(self.data, self.labels, idx, self.pad, self.augment, self.seed, epoch,
                                           self.mean, self.std)
            xm, _, ybr, lr = mix_reference(xr, yr, p)
            x.copy_(xm)
            ya.copy_(yr)
            yb.copy_(ybr)
            lam.copy_(lr)
        return x, ya, yb, lam


class DeviceCachedDataset:
    """A deterministic map-style dataset (items: tensors, numbers or dicts of them) stacked once
    into device tensors; ``batch`` gathers by index (dict items come back as dicts)."""

    def __init__(self, dataset, device):
        self.device = torch.device(device)
        items = [dataset[i] for i in range(len(dataset))]
        if not items:
            raise ValueError("empty dataset")
        self.keys = list(items[0].keys()) if isinstance(items[0], dict) else None
        fields = self.keys if self.keys is not None else range(len(items[0]) if isinstance(items[0], (tuple, list))
                                                               else 1)

        def get(it, k):
            if self.keys is not None:
                return it[k]
            return it[k] if isinstance(it, (tuple, list)) else it

        self.fields = [torch.stack([torch.as_tensor(get(it, k)) for it in items]).to(self.device) for k in fields]
        self.N = len(items)

    def __len__(self):
        return self.N

    def batch(self, idx: torch.Tensor, epoch: int = 0, out=None):
        vals = [f.index_select(0, idx) for f in self.fields]
        if out is not None:
            for o, v in zip(out, vals):
                o.copy_(v)
            vals = list(out)
        if self.keys is not None:
            return dict(zip(self.keys, vals))
        return vals[0] if len(vals) == 1 else tuple(vals)


class DeviceSegDataset:
    """``{'image', 'mask'}`` items (image fp32 [C, H, W]; mask [H, W], float32 or int64 class indices) stacked
    once on ``device`` as :class:`DeviceCachedDataset` stacks them; ``batch`` gathers by index AND augments, one
    kernel (``csrc/kernels/seg_aug.hip``): flip, scale, rotate, translate as ``aug`` says, bilinear for the image,
    nearest for the mask (``data/seg_aug.py``), into ``out_size = (Ho, Wo)`` (default: the source size).  The
    epoch's parameter table is drawn on the host and copied to the device when the epoch changes -- one small
    copy per epoch, none per step.  Mask pixels from outside the source are ``mask_fill`` (default 0.0 for float
    masks; int64 masks must name theirs, usually the loss's ignore_index).  On a CPU device ``batch`` runs
    :func:`seg_aug_reference`."""

    def __init__(self, dataset, device, aug: SegAugConfig, seed=0, out_size=None, mask_fill=None):
        self.device = torch.device(device)
        items = [dataset[i] for i in range(len(dataset))]
        if not items:
            raise ValueError("empty dataset")
        if not (isinstance(items[0], dict) and "image" in items[0] and "mask" in items[0]):
            raise ValueError("DeviceSegDataset takes a dataset of {'image', 'mask'} items")
        self.keys = ["image", "mask"]
        self.images = torch.stack([torch.as_tensor(it["image"]) for it in items]).to(self.device)
        self.masks = torch.stack([torch.as_tensor(it["mask"]) for it in items]).to(self.device)
        if self.images.dtype != torch.float32 or self.images.dim() != 4:
            raise ValueError(f"images must be float32 [C, H, W], got {self.images.dtype} "
                             f"{tuple(self.images.shape[1:])}")
        self.N, self.C, self.H, self.W = self.images.shape
        if self.masks.dtype not in (torch.float32, torch.int64) or tuple(self.masks.shape) != (self.N, self.H, self.W):
            raise ValueError(f"masks must be float32 or int64 [{self.H}, {self.W}], got {self.masks.dtype} "
                             f"{tuple(self.masks.shape[1:])}")
        if not isinstance(aug, SegAugConfig):
            raise TypeError("aug must be a SegAugConfig")
        if mask_fill is None:
            if self.masks.dtype == torch.int64:
                raise ValueError("int64 masks have no default mask_fill: name one (the loss's ignore_index)")
            mask_fill = 0.0
        elif self.masks.dtype == torch.int64 and int(mask_fill) != mask_fill:
            raise ValueError(f"mask_fill of int64 masks must be an integer, got {mask_fill}")
        self.mask_fill = int(mask_fill) if self.masks.dtype == torch.int64 else float(mask_fill)
        self.Ho, self.Wo = (self.H, self.W) if out_size is None else (int(out_size[0]), int(out_size[1]))
        if self.Ho < 1 or self.Wo < 1:
            raise ValueError(f"out_size must be at least (1, 1), got {out_size}")
        self.aug, self.seed = aug, seed
        self.redraws = 0                 # tables drawn (and copied to the device) so far
        self._epoch = self._table = self._table_np = None
        self._native = None
        if self.device.type == "cuda":
            from .._ext import native

            self._native = native()

    def __len__(self):
        return self.N

    def table(self, epoch: int) -> torch.Tensor:
        """The parameter table of ``epoch`` on the device, int32 [N, 6]; redrawn when the epoch changes."""
        if self._epoch != int(epoch):
            self._table_np = draw_seg_aug(self.aug, self.seed, int(epoch), self.N, self.H, self.W, self.Ho, self.Wo)
            self._table = torch.from_numpy(self._table_np).to(self.device)
            self._epoch = int(epoch)
            self.redraws += 1
        return self._table

    def batch(self, idx: torch.Tensor, epoch: int = 0, out=None):
        """idx: int64 dataset indices on the device -> {'image': fp32 [B, C, Ho, Wo], 'mask': [B, Ho, Wo]},
        written into ``out = (x, y)`` when given."""
        B = idx.numel()
        if out is None:
            x = torch.empty(B, self.C, self.Ho, self.Wo, dtype=torch.float32, device=self.device)
            y = torch.empty(B, self.Ho, self.Wo, dtype=self.masks.dtype, device=self.device)
        else:
            x, y = out
            if tuple(x.shape) != (B, self.C, self.Ho, self.Wo) or tuple(y.shape) != (B, self.Ho, self.Wo):
                raise ValueError(f"out must be ([{B}, {self.C}, {self.Ho}, {self.Wo}], [{B}, {self.Ho}, {self.Wo}]), "
                                 f"got {tuple(x.shape)} and {tuple(y.shape)}")
        table = self.table(epoch)
        if self._native is not None:
            self._native.seg_aug_batch(self.images, self.masks, idx, table, self.aug.image_fill, self.mask_fill, x, y)
        else:
            xr, yr = seg_aug_reference(self.images, self.masks, idx, self._table_np, self.Ho, self.Wo,
                                       self.aug.image_fill, self.mask_fill)
            x.copy_(xr)
            y.copy_(yr)
        return {"image": x, "mask": y}


class DeviceBatches:
    """Batches of a device-resident dataset in ``sampler`` order (a DistributedSampler: this rank's
    shard, shuffled by seed + epoch), or in order without a sampler.  ``out``: fixed tensors every
    full batch is written into (for a captured training step)."""

    def __init__(self, dataset, batch_size, sampler=None, drop_last=False, out=None):
        self.ds, self.bs, self.sampler, self.drop_last, self.out = dataset, batch_size, sampler, drop_last, out
        self.mixed = getattr(dataset, "mix", None) is not None   # batches are (x, labels_a, labels_b, lam)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.ds)
        return n // self.bs if self.drop_last else (n + self.bs - 1) // self.bs

    def __iter__(self):
        order = list(iter(self.sampler)) if self.sampler is not None else list(range(len(self.ds)))
        epoch = getattr(self.sampler, "epoch", 0)
        idx = torch.tensor(order, dtype=torch.int64).to(self.ds.device, non_blocking=True)
        n = idx.numel()
        rank = getattr(self.sampler, "rank", 0)
        for no, s in enumerate(range(0, n, self.bs)):
            e = min(n, s + self.bs)
            if e - s < self.bs and self.drop_last:
                break
            full = e - s == self.bs
            out = self.out if (full and self.out is not None) else None
            if self.mixed:   # the mix is drawn per (seed, epoch, rank, batch number)
                yield self.ds.batch(idx[s:e], epoch, out=out, batch_no=no, rank=rank)
            else:
                yield self.ds.batch(idx[s:e], epoch, out=out)
