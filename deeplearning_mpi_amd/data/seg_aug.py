"""Geometric augmentation of image / mask pairs for the segmentation trainer: flip, scale, rotate, translate
(and, with an output size other than the source's, crop and zoom), sampled on the device.

An augmented sample is an inverse affine map from output pixel ``(y, x)`` of an ``Ho x Wo`` output to source
coordinates in the ``H x W`` image, everything about the image centres, pixel centres at ``+0.5``::

    u = su (x + 0.5 - Wo/2),   v = sv (y + 0.5 - Ho/2)          su, sv = -1 when flipped, else 1
    x_src = (cos t u - sin t v) / s + W/2 + tx - 0.5
    y_src = (sin t u + cos t v) / s + H/2 + ty - 0.5

The host forms the six coefficients of ``x_src = a x + b y + c``, ``y_src = d x + e y + f`` in fp64 and rounds
each to Q16 (``np.rint(v * 65536)`` as int32).  From there ALL coordinate arithmetic is integer, the same on the
device (``csrc/kernels/seg_aug.hip``) and in :func:`seg_aug_reference`:

* ``X = a x + b y + c``, ``Y = d x + e y + f`` in int64;
* mask (nearest): ``ix = (X + 32768) >> 16`` (arithmetic shift: a tie rounds up), ``iy`` likewise; inside the
  image the mask value is copied, outside it is ``mask_fill``;
* image (bilinear): ``x0 = X >> 16``, ``fx = (X & 0xFFFF) / 65536`` (exact in fp32), likewise ``y0, fy``; the value
  is ``(1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11)`` in fp32 and a tap outside the image reads
  ``image_fill``.

So the mask is bit-exact between the two, the image differs by the fp32 rounding of three lerps, and identity,
flips, integer translations and 90 degree rotations (``fx = fy = 0``) are bit-exact as well.

The parameters of an epoch are ONE table, int32 ``[N, 6]``, row ``i`` for dataset index ``i``, drawn on the host
from ``np.random.default_rng([seed, epoch])`` (:func:`draw_seg_aug`): a sample's augmentation is a function of
``(seed, epoch, index)`` alone -- not of the batch size, the rank count or its place in the batch -- and a resumed
run repeats it.  The table goes to the device once per epoch; no device RNG is involved.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

Q = 65536          # Q16: one source pixel
IDENTITY = (Q, 0, 0, 0, Q, 0)


@dataclass(frozen=True)
class SegAugConfig:
    """``hflip`` / ``vflip``: probabilities of a flip; ``scale``: log-uniform in ``[lo, hi]``; ``rotate``: the angle
    uniform in +-``rotate`` degrees; ``translate``: tx, ty uniform in +-``translate`` * W and * H; with probability
    ``1 - prob`` a sample keeps only its flips; ``image_fill``: the image value outside the source."""
    hflip: float = 0.0
    vflip: float = 0.0
    scale: Tuple[float, float] = (1.0, 1.0)
    rotate: float = 0.0
    translate: float = 0.0
    prob: float = 1.0
    image_fill: float = 0.0

    def __post_init__(self):
        for n in ("hflip", "vflip", "prob"):
            v = getattr(self, n)
            if not 0 <= v <= 1:
                raise ValueError(f"{n} must lie in [0, 1], got {v}")
        try:
            lo, hi = (float(v) for v in self.scale)
        except (TypeError, ValueError):
            raise ValueError(f"scale must be a pair (lo, hi), got {self.scale!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
            raise ValueError(f"scale must satisfy 0 < lo <= hi, got {self.scale}")
        object.__setattr__(self, "scale", (lo, hi))
        for n in ("rotate", "translate"):
            v = getattr(self, n)
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"{n} must be finite and >= 0, got {v}")
        if not math.isfinite(self.image_fill):
            raise ValueError(f"image_fill must be finite, got {self.image_fill}")

    @property
    def enabled(self) -> bool:
        return self != SegAugConfig()


def _affine_q16(H, W, Ho, Wo, hflip, vflip, scale, degrees, tx, ty) -> np.ndarray:
    """The Q16 coefficients (a, b, c, d, e, f) of the transforms given as arrays (or scalars): int32 [..., 6]."""
    su = np.where(np.asarray(hflip, dtype=bool), -1.0, 1.0)
    sv = np.where(np.asarray(vflip, dtype=bool), -1.0, 1.0)
    s = np.asarray(scale, dtype=np.float64)
    if not (np.all(np.isfinite(s)) and np.all(s > 0)):
        raise ValueError("the scale of a transform must be finite and > 0")
    t = np.deg2rad(np.asarray(degrees, dtype=np.float64))
    cos, sin = np.cos(t), np.sin(t)
    tx, ty = np.asarray(tx, dtype=np.float64), np.asarray(ty, dtype=np.float64)
    a, b = cos * su / s, -sin * sv / s
    d, e = sin * su / s, cos * sv / s
    u0, v0 = 0.5 - Wo / 2.0, 0.5 - Ho / 2.0          # u = su (x + u0), v = sv (y + v0)
    c = a * u0 + b * v0 + W / 2.0 + tx - 0.5
    f = d * u0 + e * v0 + H / 2.0 + ty - 0.5
    m = np.rint(np.stack(np.broadcast_arrays(a, b, c, d, e, f), axis=-1) * Q)
    if not np.all(np.abs(m) < 2.0 ** 31):             # (NaN fails the comparison too)
        raise ValueError("a coefficient of the transform does not fit Q16 in int32")
    return m.astype(np.int32)


def seg_affine(H, W, Ho, Wo, hflip=False, vflip=False, scale=1.0, degrees=0.0, tx=0.0, ty=0.0):
    """The Q16 matrix ``(a, b, c, d, e, f)`` of one explicit transform, as six Python ints."""
    for n, v in (("H", H), ("W", W), ("Ho", Ho), ("Wo", Wo)):
        if int(v) != v or v < 1:
            raise ValueError(f"{n} must be an integer >= 1, got {v}")
    return tuple(int(v) for v in _affine_q16(H, W, Ho, Wo, hflip, vflip, float(scale), float(degrees), float(tx),
                                             float(ty)))


def draw_seg_params(cfg: SegAugConfig, seed: int, epoch: int, N: int, H: int, W: int) -> dict:
    """The transforms of ``epoch`` before they become matrices: arrays [N] ``hflip``, ``vflip`` (bool), ``scale``,
    ``degrees``, ``tx``, ``ty`` (fp64).  One ``[N, 7]`` block of uniforms -- hflip, vflip, apply, scale, angle, tx,
    ty -- is always drawn whole, so the stream does not depend on the config, and since the block fills row by
    row, row ``i`` does not depend on ``N`` either."""
    u = np.random.default_rng([int(seed), int(epoch)]).random((int(N), 7))
    apply = u[:, 2] < cfg.prob
    lo, hi = math.log(cfg.scale[0]), math.log(cfg.scale[1])
    scale = np.clip(np.exp(lo + u[:, 3] * (hi - lo)), cfg.scale[0], cfg.scale[1])
    return {"hflip": u[:, 0] < cfg.hflip, "vflip": u[:, 1] < cfg.vflip,
            "scale": np.where(apply, scale, 1.0),
            "degrees": np.where(apply, (2 * u[:, 4] - 1) * cfg.rotate, 0.0),
            "tx": np.where(apply, (2 * u[:, 5] - 1) * cfg.translate * W, 0.0),
            "ty": np.where(apply, (2 * u[:, 6] - 1) * cfg.translate * H, 0.0)}


def draw_seg_aug(cfg: SegAugConfig, seed: int, epoch: int, N: int, H: int, W: int, Ho: int, Wo: int) -> np.ndarray:
    """The parameter table of ``epoch``: int32 [N, 6], row ``i`` the Q16 matrix of dataset index ``i``."""
    p = draw_seg_params(cfg, seed, epoch, N, H, W)
    return _affine_q16(H, W, Ho, Wo, p["hflip"], p["vflip"], p["scale"], p["degrees"], p["tx"], p["ty"]).reshape(N, 6)


def _taps(src, inside, iy, ix, W, fill):
    """src [B, P, H * W] sampled at (iy, ix) [B, Ho * Wo] where ``inside``, ``fill`` elsewhere -> [B, P, Ho * Wo]."""
    flat = torch.where(inside, iy * W + ix, torch.zeros_like(ix))     # no out-of-range index is ever formed
    got = src.gather(2, flat.unsqueeze(1).expand(-1, src.shape[1], -1))
    fill = torch.full((), fill if src.dtype.is_floating_point else int(fill), dtype=src.dtype)
    return torch.where(inside.unsqueeze(1), got, fill)


def seg_aug_reference(images, masks, idx, table, Ho, Wo, image_fill=0.0, mask_fill=0, dtype=torch.float32):
    """Torch reference of the batch kernel (and the CPU execution path): images fp32 [N, C, H, W], masks [N, H, W],
    idx int64 [B], table int32 [N, 6] -> (image ``dtype`` [B, C, Ho, Wo], mask [B, Ho, Wo] of the masks' dtype).
    ``dtype``: torch.float32 (the device's arithmetic) or torch.float64."""
    idx = torch.as_tensor(idx).to(torch.int64).cpu()
    images, masks = torch.as_tensor(images), torch.as_tensor(masks)
    N, C, H, W = images.shape
    table = torch.as_tensor(np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table))
    if tuple(table.shape) != (N, 6) or tuple(masks.shape) != (N, H, W):
        raise ValueError(f"table must be [{N}, 6] and masks [{N}, {H}, {W}], got {tuple(table.shape)} and "
                         f"{tuple(masks.shape)}")
    B = idx.numel()
    t = table.to(torch.int64)[idx]                                       # [B, 6]
    a, b, c, d, e, f = (t[:, k].view(B, 1, 1) for k in range(6))
    xs = torch.arange(Wo, dtype=torch.int64).view(1, 1, Wo)
    ys = torch.arange(Ho, dtype=torch.int64).view(1, Ho, 1)
    X = (a * xs + b * ys + c).reshape(B, Ho * Wo)
    Y = (d * xs + e * ys + f).reshape(B, Ho * Wo)

    def inside(iy, ix):
        return (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)

    src_m = masks.cpu()[idx].reshape(B, 1, H * W)
    ix, iy = (X + Q // 2) >> 16, (Y + Q // 2) >> 16
    mask = _taps(src_m, inside(iy, ix), iy, ix, W, mask_fill).view(B, Ho, Wo)

    src = images.cpu()[idx].to(dtype).reshape(B, C, H * W)
    x0, y0 = X >> 16, Y >> 16
    fx = ((X & 0xFFFF).to(dtype) / Q).unsqueeze(1)
    fy = ((Y & 0xFFFF).to(dtype) / Q).unsqueeze(1)
    p00 = _taps(src, inside(y0, x0), y0, x0, W, image_fill)
    p01 = _taps(src, inside(y0, x0 + 1), y0, x0 + 1, W, image_fill)
    p10 = _taps(src, inside(y0 + 1, x0), y0 + 1, x0, W, image_fill)
    p11 = _taps(src, inside(y0 + 1, x0 + 1), y0 + 1, x0 + 1, W, image_fill)
    image = (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11)
    return image.view(B, C, Ho, Wo), mask
