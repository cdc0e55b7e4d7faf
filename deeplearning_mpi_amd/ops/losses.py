"""Fused losses and evaluation metrics (HIP kernels on GPU, torch reference on CPU).

``CrossEntropyLoss`` / ``BCEWithLogitsLoss`` are drop-in for the torch modules the reference uses
(/root/reference/pytorch/resnet/main.py:113, /root/reference/pytorch/unet/train.py:162) for the
``reduction='mean'`` case: one kernel for the loss, one for the gradient, deterministic reductions.
``ce_dice_loss`` / ``bce_dice_loss`` / ``dice_loss`` add the differentiable soft Dice of segmentation
training, computed in the same passes over the logits as the cross-entropy / BCE alone.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .backend import make_backend, pixel_strides

_BE = {}
_ONES = {}


def backward(loss: torch.Tensor):
    """``loss.backward()`` with a cached unit seed gradient (autograd's own seed is an ATen fill
    launch every step; with this the training step launches our kernels only)."""
    key = (loss.device, loss.dtype)
    one = _ONES.get(key)
    if one is None:
        one = _ONES[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
    loss.backward(one)


def _be(device, dtype=None):
    dt = torch.float64 if dtype == torch.float64 else torch.float32
    key = (str(device), dt)
    b = _BE.get(key)
    if b is None:
        b = _BE[key] = make_backend(device, dt)
    return b


class _CE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        logits = logits.contiguous()
        be = _be(logits.device, logits.dtype)
        loss, lse = be.ce_fwd(logits.to(be.dt), labels)
        ctx.save_for_backward(logits, labels, lse)
        return loss

    @staticmethod
    def backward(ctx, go):
        logits, labels, lse = ctx.saved_tensors
        be = _be(logits.device, logits.dtype)
        g = be.ce_bwd(logits.to(be.dt), labels, lse, go.reshape(1).to(be.dt).contiguous())
        return g.to(logits.dtype), None


class _BCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        logits = logits.contiguous()
        target = target.contiguous().to(_be(logits.device, logits.dtype).dt)
        be = _be(logits.device, logits.dtype)
        loss = be.bce_fwd(logits.to(be.dt), target)
        ctx.save_for_backward(logits, target)
        return loss

    @staticmethod
    def backward(ctx, go):
        logits, target = ctx.saved_tensors
        be = _be(logits.device, logits.dtype)
        g = be.bce_bwd(logits.to(be.dt), target, go.reshape(1).to(be.dt).contiguous())
        return g.view(logits.shape).to(logits.dtype), None


def _pixel_layout(logits):
    """The logits as the pixel kernels address them: unchanged in the two native layouts (contiguous
    NCHW, or the engine's NHWC buffer viewed as NCHW), else a contiguous copy."""
    return logits if pixel_strides(logits) is not None else logits.contiguous()


def _pixel_inputs(logits, labels, weight):
    """-> (backend, logits in a native layout, contiguous labels, contiguous weight or None) of a pixel-wise loss."""
    be = _be(logits.device, logits.dtype)
    w = weight.to(be.dt).contiguous() if weight is not None else None
    return be, _pixel_layout(logits).to(be.dt), labels.contiguous(), w


class _PixelCE(torch.autograd.Function):
    """Pixel-wise softmax cross-entropy: logits [N, K, H, W] (read in place, no copy), labels int64
    [N, H, W]; the gradient comes back in the strides of the logits."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index):
        be, x, labels, w = _pixel_inputs(logits, labels, weight)
        loss, lse, den = be.pixel_ce_fwd(x, labels, w, ignore_index)
        ctx.save_for_backward(x, labels, lse, den, w)
        ctx.ignore_index = ignore_index
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        x, labels, lse, den, w = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        g = be.pixel_ce_bwd(x, labels, lse, den, go.reshape(1).to(be.dt).contiguous(), w, ctx.ignore_index)
        return g.to(ctx.in_dtype), None, None, None


def _check_pixel_args(logits, labels, weight=None):
    if labels.dim() != 3 or labels.dtype != torch.int64 or labels.shape != logits.shape[:1] + logits.shape[2:]:
        raise ValueError(f"pixel-wise logits {tuple(logits.shape)} need int64 labels [N, H, W], got "
                         f"{labels.dtype} {tuple(labels.shape)}")
    if not 2 <= logits.shape[1] <= 256:
        raise ValueError(f"pixel-wise losses and counts take 2..256 classes, got {logits.shape[1]}")
    if weight is not None and weight.numel() != logits.shape[1]:
        raise ValueError(f"weight has {weight.numel()} entries for {logits.shape[1]} classes")


class _ClsCE(torch.autograd.Function):
    """Classification cross-entropy with weight / ignore_index / label smoothing and two-label mixed targets
    (csrc/kernels/cls_ce.hip).  ``labels_b`` and ``lam`` are read in place by both passes, so a replayed graph
    follows what they hold at replay time; the buffers are ``empty`` and no ATen kernel is launched."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, label_smoothing, labels_b, lam):
        be = _be(logits.device, logits.dtype)
        x = logits.contiguous().to(be.dt)
        w = weight.to(be.dt).contiguous() if weight is not None else None
        lam = lam.to(be.dt) if lam is not None else None
        loss, lse, rows, den = be.cls_ce_fwd(x, labels, w, ignore_index, label_smoothing, labels_b, lam)
        ctx.save_for_backward(x, labels, lse, rows, den, w, labels_b, lam)
        ctx.ignore_index, ctx.label_smoothing, ctx.in_dtype = ignore_index, label_smoothing, logits.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        x, labels, lse, rows, den, w, labels_b, lam = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        g = be.cls_ce_bwd(x, labels, lse, rows, den, go.reshape(1).to(be.dt).contiguous(), w, ctx.ignore_index,
                          ctx.label_smoothing, labels_b, lam)
        return (g.to(ctx.in_dtype),) + (None,) * 6


def _check_cls_args(logits, labels, weight, label_smoothing, labels_b, lam):
    if logits.dim() != 2:
        raise ValueError(f"cross_entropy takes [N, K] or [N, K, H, W] logits, got {tuple(logits.shape)}")
    N, K = logits.shape
    if (labels_b is None) != (lam is None):
        raise ValueError("labels_b and lam come together: a mixed target needs both")
    for name, y in (("labels", labels), ("labels_b", labels_b)):
        if y is not None and (y.dtype != torch.int64 or y.shape != (N,)):
            raise ValueError(f"[N, K] logits need int64 {name} [N], got {y.dtype} {tuple(y.shape)}")
    if lam is not None and (not torch.is_tensor(lam) or not lam.is_floating_point() or lam.numel() not in (1, N)
                            or lam.device != logits.device):
        raise ValueError("lam must be a float tensor of 1 or N elements on the device of the logits")
    if weight is not None and weight.numel() != K:
        raise ValueError(f"weight has {weight.numel()} entries for {K} classes")
    if not (math.isfinite(label_smoothing) and 0 <= label_smoothing < 1):
        raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing}")


def cross_entropy(logits, labels, weight=None, ignore_index=-100, label_smoothing=0.0, labels_b=None, lam=None):
    """Mean softmax cross-entropy.  [N, K] logits with [N] labels: the classification loss;
    [N, K, H, W] logits with [N, H, W] labels: the pixel-wise loss.  Both take torch's ``weight`` /
    ``ignore_index`` semantics (labels outside [0, K) are ignored as well).

    The classification loss also takes ``label_smoothing`` (torch's) and a two-label mixed target for mixup /
    CutMix: ``labels_b`` int64 [N] with ``lam``, a float32 tensor of 1 or N elements on the device.  With
    keep(y) = y is neither ``ignore_index`` nor outside [0, K):
    t[c] = lam [a = c] keep(a) + (1 - lam) [b = c] keep(b), m = lam keep(a) + (1 - lam) keep(b),
    q[c] = (1 - eps) t[c] + (eps / K) m, and loss = - sum_n sum_c w_c q_n[c] log softmax_n[c] / sum_n sum_c w_c t_n[c]
    (NaN when nothing is kept, as torch).  ``lam`` stays on the device -- a replayed graph reads its current
    value -- and is trusted to lie in [0, 1]: checking it would need a host synchronisation.
    A call with every default runs the plain classification kernels (mean over N)."""
    if logits.dim() == 4:
        if label_smoothing != 0 or labels_b is not None or lam is not None:
            raise NotImplementedError("label_smoothing / labels_b / lam are implemented for classification ([N, K]) "
                                      "logits, not for pixel-wise ([N, K, H, W]) logits")
        _check_pixel_args(logits, labels, weight)
        return _PixelCE.apply(logits, labels, weight, int(ignore_index))
    if weight is None and ignore_index == -100 and label_smoothing == 0 and labels_b is None and lam is None:
        return _CE.apply(logits, labels)
    label_smoothing = float(label_smoothing)
    _check_cls_args(logits, labels, weight, label_smoothing, labels_b, lam)
    return _ClsCE.apply(logits, labels, weight, int(ignore_index), label_smoothing, labels_b, lam)


def bce_with_logits(logits, target):
    return _BCE.apply(logits, target)


class _PixelCEDice(torch.autograd.Function):
    """ce_weight * pixel-wise cross-entropy + dice_weight * soft Dice in the passes of _PixelCE: one fused
    forward, one finish, one fused backward; logits read in place, gradient in their strides."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, ce_weight, dice_weight, smooth, include_background):
        be, x, labels, w = _pixel_inputs(logits, labels, weight)
        loss, lse, den, tab = be.pixel_ce_dice_fwd(x, labels, w, ignore_index, ce_weight, dice_weight, smooth,
                                                   include_background)
        ctx.save_for_backward(x, labels, lse, den, tab, w)
        ctx.ignore_index, ctx.ce_weight, ctx.in_dtype = ignore_index, ce_weight, logits.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        x, labels, lse, den, tab, w = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        g = be.pixel_ce_dice_bwd(x, labels, lse, den, tab, go.reshape(1).to(be.dt).contiguous(), w, ctx.ignore_index,
                                 ctx.ce_weight)
        return (g.to(ctx.in_dtype),) + (None,) * 7


class _BCEDice(torch.autograd.Function):
    """bce_weight * BCE-with-logits + dice_weight * soft Dice of sigmoid(logits), per sample [N, ...]."""

    @staticmethod
    def forward(ctx, logits, target, bce_weight, dice_weight, smooth):
        be = _be(logits.device, logits.dtype)
        x = logits.contiguous().to(be.dt)
        target = target.contiguous().to(be.dt)
        loss, tab = be.bce_dice_fwd(x, target, bce_weight, dice_weight, smooth)
        ctx.save_for_backward(x, target, tab)
        ctx.bce_weight, ctx.in_dtype = bce_weight, logits.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        x, target, tab = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        g = be.bce_dice_bwd(x, target, tab, go.reshape(1).to(be.dt).contiguous(), ctx.bce_weight)
        return g.view(x.shape).to(ctx.in_dtype), None, None, None, None


def _check_dice_args(w0, w1, smooth, names):
    for v, n in ((w0, names[0]), (w1, names[1])):
        if not math.isfinite(v) or v < 0:
            raise ValueError(f"{n} must be finite and >= 0, got {v}")
    if w0 == 0 and w1 == 0:
        raise ValueError(f"{names[0]} and {names[1]} must not both be 0")
    if not (math.isfinite(smooth) and smooth > 0):
        raise ValueError(f"smooth must be > 0 (it keeps an empty sample at dice = 1), got {smooth}")


def ce_dice_loss(logits, labels, weight=None, ignore_index=-100, ce_weight=1.0, dice_weight=1.0, smooth=1.0,
                 include_background=True):
    """``ce_weight * CE + dice_weight * (1 - mean dice)`` for [N, K, H, W] logits and int64 [N, H, W] labels.
    CE is :func:`cross_entropy` (``weight`` applies to it only); dice[n, c] = (2 I + smooth) / (P + T + smooth)
    with I = sum p_c [y = c], P = sum p_c, T = sum [y = c] over the kept pixels of sample n (p the softmax,
    kept as in CE), averaged over the samples and all classes (``include_background=False``: classes 1..K-1).
    A sample without kept pixels has dice 1.  On the GPU the Dice sums and gradient ride in the CE kernels'
    passes; ``dice_weight=0`` is :func:`cross_entropy` itself."""
    ce_weight, dice_weight, smooth = float(ce_weight), float(dice_weight), float(smooth)
    _check_dice_args(ce_weight, dice_weight, smooth, ("ce_weight", "dice_weight"))
    if logits.dim() != 4:
        raise ValueError(f"ce_dice_loss takes [N, K, H, W] logits, got {tuple(logits.shape)}")
    _check_pixel_args(logits, labels, weight)
    if dice_weight == 0:
        loss = _PixelCE.apply(logits, labels, weight, int(ignore_index))
        return loss if ce_weight == 1 else loss * ce_weight
    return _PixelCEDice.apply(logits, labels, weight, int(ignore_index), ce_weight, dice_weight, smooth,
                              bool(include_background))


def bce_dice_loss(logits, target, bce_weight=1.0, dice_weight=1.0, smooth=1.0):
    """``bce_weight * BCE + dice_weight * (1 - mean_n dice[n])`` for logits [N, H, W] or [N, 1, H, W] and a
    float target [N, H, W] in [0, 1]: p = sigmoid(logits), dice[n] = (2 sum p t + smooth) / (sum p + sum t +
    smooth).  ``dice_weight=0`` is :func:`bce_with_logits` itself."""
    bce_weight, dice_weight, smooth = float(bce_weight), float(dice_weight), float(smooth)
    _check_dice_args(bce_weight, dice_weight, smooth, ("bce_weight", "dice_weight"))
    if logits.dim() == target.dim() + 1 and logits.shape[1] == 1:
        logits = logits.squeeze(1)
    if target.dim() < 2 or logits.shape != target.shape or not target.is_floating_point():
        raise ValueError(f"bce_dice_loss takes logits [N, H, W] or [N, 1, H, W] and a float target [N, H, W], got "
                         f"{tuple(logits.shape)} and {target.dtype} {tuple(target.shape)}")
    if dice_weight == 0:
        loss = _BCE.apply(logits, target)
        return loss if bce_weight == 1 else loss * bce_weight
    return _BCEDice.apply(logits, target, bce_weight, dice_weight, smooth)


def dice_loss(logits, target, smooth=1.0, include_background=True, ignore_index=-100):
    """The soft Dice loss alone: int64 class-index targets -> the softmax form of :func:`ce_dice_loss`
    (``ce_weight=0``), float targets -> the sigmoid form of :func:`bce_dice_loss` (``bce_weight=0``)."""
    if target.dtype == torch.int64:
        return ce_dice_loss(logits, target, None, ignore_index, 0.0, 1.0, smooth, include_background)
    if target.is_floating_point():
        return bce_dice_loss(logits, target, 0.0, 1.0, smooth)
    raise ValueError(f"dice_loss takes int64 class indices or a float target, got {target.dtype}")


class CEDiceLoss(nn.Module):
    def __init__(self, weight=None, ignore_index=-100, ce_weight=1.0, dice_weight=1.0, smooth=1.0,
                 include_background=True):
        super().__init__()
        self.register_buffer("weight", weight)
        self.ignore_index, self.ce_weight, self.dice_weight = ignore_index, ce_weight, dice_weight
        self.smooth, self.include_background = smooth, include_background

    def forward(self, logits, labels):
        return ce_dice_loss(logits, labels, self.weight, self.ignore_index, self.ce_weight, self.dice_weight,
                            self.smooth, self.include_background)


class BCEDiceLoss(nn.Module):
    def __init__(self, bce_weight=1.0, dice_weight=1.0, smooth=1.0):
        super().__init__()
        self.bce_weight, self.dice_weight, self.smooth = bce_weight, dice_weight, smooth

    def forward(self, logits, target):
        return bce_dice_loss(logits, target, self.bce_weight, self.dice_weight, self.smooth)


class DiceLoss(nn.Module):
    def __init__(self, smooth=1.0, include_background=True, ignore_index=-100):
        super().__init__()
        self.smooth, self.include_background, self.ignore_index = smooth, include_background, ignore_index

    def forward(self, logits, target):
        return dice_loss(logits, target, self.smooth, self.include_background, self.ignore_index)


class CrossEntropyLoss(nn.Module):
    def __init__(self, weight=None, ignore_index=-100, label_smoothing=0.0):
        super().__init__()
        self.register_buffer("weight", weight)
        self.ignore_index, self.label_smoothing = ignore_index, label_smoothing

    def forward(self, logits, labels, labels_b=None, lam=None):
        return cross_entropy(logits, labels, self.weight, self.ignore_index, self.label_smoothing, labels_b, lam)


class BCEWithLogitsLoss(nn.Module):
    def forward(self, logits, target):
        return bce_with_logits(logits, target)


@torch.no_grad()
def top1_correct(logits, labels) -> torch.Tensor:
    """Device int32[1] count of argmax(logits) == labels (reference main.py:65-71)."""
    return _be(logits.device, logits.dtype).argmax_correct(logits.float().contiguous(), labels)


@torch.no_grad()
def dice_per_sample(logits, target) -> torch.Tensor:
    """Per-sample Dice of (sigmoid(logits) > 0.5) vs target, 1.0 when both are empty
    (reference train.py:121-137).  logits [N,1,H,W] or [N,H,W]; target [N,H,W]."""
    lg = logits.reshape(target.shape).float().contiguous()
    return _be(logits.device, logits.dtype).dice(lg, target.float().contiguous())


@torch.no_grad()
def seg_counts(logits, labels, ignore_index=-100) -> torch.Tensor:
    """int64 [N, K, 3]: per sample and class c the exact pixel counts {|pred = c and target = c|,
    |pred = c|, |target = c|}, pred = argmax over the classes (ties to the lowest index).  Pixels whose
    label is ``ignore_index`` or outside [0, K) count nowhere.  logits [N, K, H, W], labels int64 [N, H, W]."""
    _check_pixel_args(logits, labels)
    be = _be(logits.device, logits.dtype)
    return be.seg_counts(_pixel_layout(logits.detach()).to(be.dt), labels.contiguous(), int(ignore_index))


@torch.no_grad()
def dice_multiclass(logits, labels, ignore_index=-100) -> torch.Tensor:
    """Per-sample Dice [N] of argmax(logits) against integer labels: the mean over the foreground
    classes 1..K-1 of (2 inter + 1e-8) / (pred + target + 1e-8); a class absent from both scores 1.0
    (the reference's empty-mask rule, train.py:133-137, per class)."""
    c = seg_counts(logits, labels, ignore_index)[:, 1:].double()
    uni = c[..., 1] + c[..., 2]
    d = torch.where(uni > 0, (2 * c[..., 0] + 1e-8) / (uni + 1e-8), torch.ones_like(uni))
    return d.mean(1).float()


@torch.no_grad()
def mean_iou(logits, labels, ignore_index=-100) -> torch.Tensor:
    """Mean intersection-over-union (scalar) of argmax(logits) against integer labels: the counts are
    summed over the batch, classes whose union is empty are left out of the mean."""
    c = seg_counts(logits, labels, ignore_index).sum(0).double()
    union = c[:, 1] + c[:, 2] - c[:, 0]
    has = union > 0
    iou = torch.where(has, c[:, 0] / union.clamp_min(1), torch.zeros_like(union))
    return (iou.sum() / has.sum()).float()
