"""mixup and CutMix of a batch with itself, for the classification recipe.

The host draws ONE mix per batch -- kind, ``lam`` and (CutMix) a box -- from
``np.random.default_rng([seed, epoch, rank, batch_no])``: a function of those four numbers alone, so a resumed
run repeats it and no device RNG is involved.  The device does the blending: fused into the batch kernel of the
device-resident pipeline (``DeviceImageDataset(mix=...)``) or in place on any fp32 NCHW batch
(:func:`mix_batch_`), both in ``csrc/kernels/data.hip``.

Sample ``b`` is mixed with sample ``B - 1 - b`` of the same batch and ``labels_b[b] = labels[B - 1 - b]``; the
loss of the mixed batch is ``ops.cross_entropy(logits, labels, labels_b=labels_b, lam=lam)``.  The middle sample
of an odd batch is its own partner and stays bit-exactly as it was, as does every sample of an unmixed batch.

* mixup:  ``out = lam * u + (1 - lam) * v`` on the normalised values, ``lam ~ Beta(alpha, alpha)``.
* CutMix: inside rows ``[y0, y1)`` and columns ``[x0, x1)`` the partner's pixel, elsewhere the sample's own; the
  box has side ratio ``sqrt(1 - lam)`` around a uniform centre, is clipped to the image, and ``lam`` is then
  recomputed as ``1 - box_area / (H * W)``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Tuple

import numpy as np
import torch

KINDS = ("none", "mixup", "cutmix")


@dataclass(frozen=True)
class MixConfig:
    """``mixup_alpha`` / ``cutmix_alpha`` > 0 switch the two on (both: CutMix with probability ``switch_prob``);
    a batch is mixed at all with probability ``prob``."""
    mixup_alpha: float = 0.0
    cutmix_alpha: float = 0.0
    prob: float = 1.0
    switch_prob: float = 0.5

    def __post_init__(self):
        for n in ("mixup_alpha", "cutmix_alpha"):
            v = getattr(self, n)
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"{n} must be finite and >= 0, got {v}")
        for n in ("prob", "switch_prob"):
            v = getattr(self, n)
            if not 0 <= v <= 1:
                raise ValueError(f"{n} must lie in [0, 1], got {v}")

    @property
    def enabled(self) -> bool:
        return (self.mixup_alpha > 0 or self.cutmix_alpha > 0) and self.prob > 0


class MixParams(NamedTuple):
    kind: str = "none"
    lam: float = 1.0
    box: Tuple[int, int, int, int] = (0, 0, 0, 0)   # y0, y1, x0, x1


def draw_mix(cfg: MixConfig, seed: int, epoch: int, rank: int, batch_no: int, H: int, W: int) -> MixParams:
    """The mix of batch ``batch_no`` of ``epoch`` on ``rank``."""
    rng = np.random.default_rng([int(seed), int(epoch), int(rank), int(batch_no)])
    u_mix, u_switch = rng.random(), rng.random()   # always drawn, so the stream does not depend on the config
    if (cfg.mixup_alpha <= 0 and cfg.cutmix_alpha <= 0) or u_mix >= cfg.prob:
        return MixParams()
    if cfg.mixup_alpha > 0 and cfg.cutmix_alpha > 0:
        cut = u_switch < cfg.switch_prob
    else:
        cut = cfg.cutmix_alpha > 0
    alpha = cfg.cutmix_alpha if cut else cfg.mixup_alpha
    lam = min(1.0, max(0.0, float(rng.beta(alpha, alpha))))
    if not cut:
        return MixParams("mixup", lam)
    ratio = math.sqrt(1.0 - lam)
    bh, bw = int(H * ratio), int(W * ratio)
    cy, cx = int(rng.integers(H)), int(rng.integers(W))
    y0, y1 = min(max(cy - bh // 2, 0), H), min(max(cy + bh // 2, 0), H)
    x0, x1 = min(max(cx - bw // 2, 0), W), min(max(cx + bw // 2, 0), W)
    return MixParams("cutmix", 1.0 - (y1 - y0) * (x1 - x0) / (H * W), (y0, y1, x0, x1))


def check_params(params: MixParams, H: int, W: int):
    y0, y1, x0, x1 = params.box
    if params.kind not in KINDS:
        raise ValueError(f"mix kind must be one of {KINDS}, got {params.kind!r}")
    if not 0 <= params.lam <= 1:
        raise ValueError(f"lam must lie in [0, 1], got {params.lam}")
    if not (0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W):
        raise ValueError(f"the box {params.box} does not lie inside the {H} x {W} image")


def mix_reference(x: torch.Tensor, labels: torch.Tensor, params: MixParams):
    """Torch reference of both device paths (and their CPU path): -> (mixed x, labels, labels_b, lam [1] fp32)."""
    B, _, H, W = x.shape
    check_params(params, H, W)
    lam = torch.tensor([params.lam], dtype=torch.float32, device=x.device)
    out, xf = x.clone(), x.flip(0)
    if params.kind == "mixup":
        out = x * lam[0].to(x.dtype) + xf * (1 - lam[0]).to(x.dtype)
        if B % 2:
            out[B // 2] = x[B // 2]   # its own partner: untouched, not blended with itself
    elif params.kind == "cutmix":
        y0, y1, x0, x1 = params.box
        out[:, :, y0:y1, x0:x1] = xf[:, :, y0:y1, x0:x1]
    return out, labels, labels.flip(0), lam


def mix_batch_(x, labels, params: MixParams, labels_b=None, lam=None):
    """Mix the fp32 batch ``x`` [B, C, H, W] in place -> (x, labels, labels_b, lam).  ``labels_b`` (int64 [B]) and
    ``lam`` (fp32 [1]) are written into when given, which keeps them the fixed inputs of a captured step.  On the
    GPU this is one kernel launch; on the CPU the torch reference."""
    B, _, H, W = x.shape
    check_params(params, H, W)
    if labels_b is None:
        labels_b = torch.empty_like(labels)
    if lam is None:
        lam = torch.empty(1, dtype=torch.float32, device=x.device)
    if x.device.type == "cuda":
        from .._ext import native

        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("mix_batch_ takes a contiguous fp32 batch")
        native().mix_batch_(x, labels.contiguous(), KINDS.index(params.kind), float(params.lam), *params.box, labels_b,
                            lam)
    else:
        xr, _, lb, lr = mix_reference(x, labels, params)
        x.copy_(xr)
        labels_b.copy_(lb)
        lam.copy_(lr)
    return x, labels, labels_b, lam
