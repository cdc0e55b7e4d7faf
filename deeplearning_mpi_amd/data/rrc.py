"""RandomResizedCrop for the device-resident classification pipeline: images stored at one size, batches
assembled at any other (``DeviceImageDataset(rrc=...)``, ``csrc/kernels/rrc.hip``).

**The box.**  A sample's crop is an integer box ``(top, left, h, w)`` inside its ``H x W`` stored image plus a flip
bit.  The boxes of an epoch are ONE table, int32 ``[N, 5]`` with rows ``(top, left, h, w, flip)``, row ``i`` for
dataset index ``i``, drawn on the host (:func:`draw_rrc`) by torchvision's ``RandomResizedCrop.get_params`` rule,
vectorised: per try ``area = H W U(scale)``, ``log r ~ U(log ratio)``, ``w = round(sqrt(area r))``,
``h = round(sqrt(area / r))``; a try is valid when ``0 < w <= W`` and ``0 < h <= H``, then
``top = floor(u (H - h + 1))`` and ``left`` likewise; the first valid try of 10 wins, and with none the centred
fallback clamps the whole image's ratio into ``ratio``.  All draws are one
``np.random.default_rng([seed, epoch]).random((N, 41))`` block (10 tries x (area, ratio, top, left), then the
flip), always drawn whole: a sample's crop is a function of ``(seed, epoch, index)`` alone -- not of the batch
size, the rank count or its place in the batch -- and a resumed run repeats it.  The table goes to the device once
per epoch; no device RNG is involved.

**The resampling.**  The resize of the ``h x w`` box to ``Ho x Wo`` is the separable anti-aliased bilinear (tent)
filter that ``F.interpolate(crop, mode="bilinear", antialias=True, align_corners=False)`` applies; it never reads
outside the box.  Per axis (``n`` source, ``m`` output pixels)::

    scale = n / m        support = max(scale, 1)        centre_i = scale (i + 0.5)
    lo_i = max(0, floor(centre_i - support + 0.5))      hi_i = min(n, floor(centre_i + support + 0.5))
    t_j  = max(0, 1 - |j - centre_i + 0.5| / support),  j in [lo_i, hi_i),  divided by their sum

``lo`` and ``hi`` are evaluated in exact integer arithmetic (both floor arguments are rationals over ``2 m``), so
the device and :func:`rrc_reference` can never disagree on a tap range; at an exact tie that rule adds or drops
only a tap of weight 0.  The weights are fp32.  The resize runs on ``u8 / 255``, rows first (x), then columns (y);
then ``(v - mean_c) / std_c``; a flip mirrors the output column; labels are gathered.  With ``h = Ho`` and
``w = Wo`` every row of weights is one 1 and one 0, so an identity crop is bit-equal to
``image_batch_reference(augment=False)``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

TRIES = 10
MAX_SCALE = 15     # the kernel's weight table holds 32 taps per output pixel and axis: h / Ho, w / Wo <= 15


@dataclass(frozen=True)
class RrcConfig:
    """``scale``: the box area as a fraction of the image, uniform in ``[lo, hi]``; ``ratio``: w / h, log-uniform
    in ``[lo, hi]``; ``hflip``: probability of a horizontal flip."""
    scale: Tuple[float, float] = (0.08, 1.0)
    ratio: Tuple[float, float] = (3 / 4, 4 / 3)
    hflip: float = 0.5

    def __post_init__(self):
        for n in ("scale", "ratio"):
            try:
                lo, hi = (float(v) for v in getattr(self, n))
            except (TypeError, ValueError):
                raise ValueError(f"{n} must be a pair (lo, hi), got {getattr(self, n)!r}") from None
            if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
                raise ValueError(f"{n} must satisfy 0 < lo <= hi, got {getattr(self, n)}")
            object.__setattr__(self, n, (lo, hi))
        if not 0 <= self.hflip <= 1:
            raise ValueError(f"hflip must lie in [0, 1], got {self.hflip}")


def draw_rrc(cfg: RrcConfig, seed: int, epoch: int, N: int, H: int, W: int) -> np.ndarray:
    """The crop table of ``epoch``: int32 [N, 5], row ``i`` = (top, left, h, w, flip) of dataset index ``i``."""
    N, H, W = int(N), int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"the stored image must be at least 1 x 1, got {H} x {W}")
    u = np.random.default_rng([int(seed), int(epoch)]).random((N, 4 * TRIES + 1))
    t = u[:, :4 * TRIES].reshape(N, TRIES, 4)
    area = H * W * (cfg.scale[0] + t[:, :, 0] * (cfg.scale[1] - cfg.scale[0]))
    lo, hi = math.log(cfg.ratio[0]), math.log(cfg.ratio[1])
    r = np.exp(lo + t[:, :, 1] * (hi - lo))
    w = np.rint(np.sqrt(area * r)).astype(np.int64)
    h = np.rint(np.sqrt(area / r)).astype(np.int64)
    valid = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    first = valid.argmax(axis=1)                       # the first valid try (0 when there is none)
    rows = np.arange(N)
    w, h = w[rows, first], h[rows, first]
    top = np.minimum(np.floor(t[rows, first, 2] * (H - h + 1)).astype(np.int64), H - h)
    left = np.minimum(np.floor(t[rows, first, 3] * (W - w + 1)).astype(np.int64), W - w)
    # the centred fallback: the whole image, its ratio clamped into `ratio`
    fh, fw = H, W
    if W / H < cfg.ratio[0]:
        fh = min(H, max(1, int(round(W / cfg.ratio[0]))))
    elif W / H > cfg.ratio[1]:
        fw = min(W, max(1, int(round(H * cfg.ratio[1]))))
    ok = valid.any(axis=1)
    table = np.stack([np.where(ok, top, (H - fh) // 2), np.where(ok, left, (W - fw) // 2), np.where(ok, h, fh),
                      np.where(ok, w, fw), u[:, 4 * TRIES] < cfg.hflip], axis=1)
    return np.ascontiguousarray(table.astype(np.int32))


def center_box(H: int, W: int, frac: float) -> Tuple[int, int, int, int, int]:
    """The evaluation box: the centred square of side ``round(frac * min(H, W))``, not flipped."""
    if not (math.isfinite(frac) and 0 < frac <= 1):
        raise ValueError(f"the centre crop fraction must lie in (0, 1], got {frac}")
    side = min(min(H, W), max(1, int(round(frac * min(H, W)))))
    return ((H - side) // 2, (W - side) // 2, side, side, 0)


def check_table(table: np.ndarray, N: int, H: int, W: int, Ho: int, Wo: int):
    """What the binding checks of a table, for the CPU path."""
    t = np.asarray(table)
    if t.dtype != np.int32 or t.shape != (N, 5):
        raise ValueError(f"the crop table must be int32 [{N}, 5], got {t.dtype} {t.shape}")
    top, left, h, w, flip = (t[:, k].astype(np.int64) for k in range(5))
    if (h < 1).any() or (w < 1).any():
        raise ValueError("a crop box has h or w < 1")
    if (top < 0).any() or (left < 0).any() or (top + h > H).any() or (left + w > W).any():
        raise ValueError(f"a crop box does not lie inside the {H} x {W} image")
    if ((flip != 0) & (flip != 1)).any():
        raise ValueError("the flip of a crop must be 0 or 1")
    if (h > MAX_SCALE * Ho).any() or (w > MAX_SCALE * Wo).any():
        raise ValueError(f"a crop box is down-scaled by more than {MAX_SCALE}x")


def rrc_taps(n: int, m: int):
    """The tap range [lo_i, hi_i) of each of ``m`` output pixels over ``n`` source pixels: two int64 [m]."""
    i = torch.arange(m, dtype=torch.int64)
    c2, s2 = n * (2 * i + 1), 2 * max(n, m)            # centre_i and support over the denominator 2 m
    lo = torch.div(c2 - s2 + m, 2 * m, rounding_mode="floor").clamp_(min=0)
    hi = torch.div(c2 + s2 + m, 2 * m, rounding_mode="floor").clamp_(max=n)
    return lo, hi


def rrc_weights(n: int, m: int, dtype=torch.float32) -> torch.Tensor:
    """The resize of one axis as a dense matrix [m, n] in ``dtype``: row ``i`` holds the normalised tent weights
    of output pixel ``i`` on its taps and zeros elsewhere."""
    lo, hi = rrc_taps(n, m)
    scale = torch.tensor(float(n), dtype=dtype) / m
    support = torch.clamp(scale, min=1.0)
    centre = scale * (torch.arange(m, dtype=dtype) + 0.5)
    j = torch.arange(n, dtype=torch.int64).view(1, n)
    t = torch.clamp(1 - ((j.to(dtype) - centre.view(m, 1)) + 0.5).abs() / support, min=0)
    t = torch.where((j >= lo.view(m, 1)) & (j < hi.view(m, 1)), t, torch.zeros((), dtype=dtype))
    return t / t.sum(dim=1, keepdim=True)


def rrc_reference(data_hwc_u8, labels, idx, table, Ho: int, Wo: int, mean, std, dtype=torch.float32):
    """Torch reference of the batch kernel (and the CPU execution path): data uint8 [N, H, W, C], labels int64 [N],
    idx int64 [B], table int32 [N, 5] -> (``dtype`` [B, C, Ho, Wo], labels [B]).  ``dtype``: torch.float32 (the
    device's arithmetic) or torch.float64."""
    idx = torch.as_tensor(idx).to(torch.int64).cpu()
    data = torch.as_tensor(data_hwc_u8).cpu()
    N, H, W, C = data.shape
    table = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table)
    check_table(table, N, H, W, Ho, Wo)
    m = torch.tensor(list(mean)[:C], dtype=torch.float32).to(dtype).view(C, 1, 1)
    s = torch.tensor(list(std)[:C], dtype=torch.float32).to(dtype).view(C, 1, 1)
    out = torch.empty(idx.numel(), C, Ho, Wo, dtype=dtype)
    for b, d in enumerate(idx.tolist()):
        top, left, h, w, flip = (int(v) for v in table[d])
        crop = data[d, top:top + h, left:left + w].permute(2, 0, 1).to(dtype) / 255.0      # [C, h, w]
        v = rrc_weights(h, Ho, dtype) @ (crop @ rrc_weights(w, Wo, dtype).t())             # rows (x), then columns
        v = (v - m) / s
        out[b] = v.flip(-1) if flip else v
    return out, torch.as_tensor(labels).cpu()[idx]
