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


_OHEM_STATS = ("cut", "k", "n_valid", "n_selected")


class _OhemCE(torch.autograd.Function):
    """:class:`_PixelCE` over the hardest pixels (csrc/kernels/ohem.hip): logits read in place, the gradient in
    their strides; returns the loss and the four device statistics (not differentiable, never read here)."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, keep_ratio, min_kept, thresh):
        be, x, labels, w = _pixel_inputs(logits, labels, weight)
        loss, lse, nll, den, st = be.ohem_ce_fwd(x, labels, w, ignore_index, keep_ratio, min_kept, thresh)
        ctx.save_for_backward(x, labels, lse, nll, st["cut"], den, w)
        ctx.ignore_index, ctx.in_dtype = ignore_index, logits.dtype
        stats = tuple(st[n] for n in _OHEM_STATS)
        ctx.mark_non_differentiable(*stats)
        return (loss,) + stats

    @staticmethod
    def backward(ctx, go, *_):
        x, labels, lse, nll, cut, den, w = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        g = be.ohem_ce_bwd(x, labels, lse, nll, cut, den, go.reshape(1).to(be.dt).contiguous(), w, ctx.ignore_index)
        return (g.to(ctx.in_dtype),) + (None,) * 6


class _OhemBCE(torch.autograd.Function):
    """BCE-with-logits over the hardest pixels: contiguous logits and float targets of one shape."""

    @staticmethod
    def forward(ctx, logits, target, keep_ratio, min_kept, thresh):
        be = _be(logits.device, logits.dtype)
        x = logits.contiguous().to(be.dt)
        target = target.contiguous().to(be.dt)
        loss, nll, den, st = be.ohem_bce_fwd(x, target, keep_ratio, min_kept, thresh)
        ctx.save_for_backward(x, target, nll, st["cut"], den)
        ctx.in_dtype = logits.dtype
        stats = tuple(st[n] for n in _OHEM_STATS)
        ctx.mark_non_differentiable(*stats)
        return (loss,) + stats

    @staticmethod
    def backward(ctx, go, *_):
        x, target, nll, cut, den = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        g = be.ohem_bce_bwd(x, target, nll, cut, den, go.reshape(1).to(be.dt).contiguous())
        return g.view(x.shape).to(ctx.in_dtype), None, None, None, None


def _check_ohem_args(keep_ratio, min_kept, thresh):
    keep_ratio, min_kept = float(keep_ratio), int(min_kept)
    if not 0 < keep_ratio <= 1:
        raise ValueError(f"keep_ratio must lie in (0, 1], got {keep_ratio}")
    if min_kept < 1:
        raise ValueError(f"min_kept must be >= 1, got {min_kept}")
    if thresh is not None and not 0 < float(thresh) < 1:
        raise ValueError(f"thresh must be None or a probability in (0, 1), got {thresh}")
    return keep_ratio, min_kept, None if thresh is None else float(thresh)


def _ohem_ce(logits, labels, weight, ignore_index, keep_ratio, min_kept, thresh):
    sel = _check_ohem_args(keep_ratio, min_kept, thresh)
    if logits.dim() != 4:
        raise ValueError(f"ohem_cross_entropy takes [N, K, H, W] logits, got {tuple(logits.shape)}")
    _check_pixel_args(logits, labels, weight)
    out = _OhemCE.apply(logits, labels, weight, int(ignore_index), *sel)
    return out[0], dict(zip(_OHEM_STATS, out[1:]))


def _ohem_bce(logits, target, keep_ratio, min_kept, thresh):
    sel = _check_ohem_args(keep_ratio, min_kept, thresh)
    if logits.dim() == target.dim() + 1 and logits.shape[1] == 1:
        logits = logits.squeeze(1)
    if target.dim() < 2 or logits.shape != target.shape or not target.is_floating_point():
        raise ValueError(f"ohem_bce_with_logits takes logits [N, H, W] or [N, 1, H, W] and a float target [N, H, W], "
                         f"got {tuple(logits.shape)} and {target.dtype} {tuple(target.shape)}")
    out = _OhemBCE.apply(logits, target, *sel)
    return out[0], dict(zip(_OHEM_STATS, out[1:]))


def ohem_cross_entropy(logits, labels, weight=None, ignore_index=-100, keep_ratio=0.25, min_kept=1, thresh=None):
    """Pixel-wise cross-entropy over the hardest pixels of the batch (online hard example mining) for
    [N, K, H, W] logits and int64 [N, H, W] labels.  With l_m = max(0, lse_m - x_m[t_m]) over the kept pixels (as
    :func:`cross_entropy`) and n_valid their number: k = min(n_valid, max(min_kept, ceil(keep_ratio * n_valid))),
    cut = the k-th largest l, or min(-log(thresh), that) with ``thresh`` (a probability: pixels predicted below
    it are always mined), S = {kept m : l_m >= cut} -- every tie at the cut included, so the set depends on no
    order -- and loss = sum_S w[t] l / sum_S w[t].  ``weight`` enters the sums only, the selection is on the
    unweighted l.  Pixels outside S get an exact zero gradient.  On the GPU k and the cut are found on the device
    by an exact radix select (csrc/kernels/ohem.hip): no host synchronisation, the same bits on every run, and
    ``keep_ratio=1, min_kept=1`` is :func:`cross_entropy`'s loss."""
    return _ohem_ce(logits, labels, weight, ignore_index, keep_ratio, min_kept, thresh)[0]


def ohem_bce_with_logits(logits, target, keep_ratio=0.25, min_kept=1, thresh=None):
    """The binary form of :func:`ohem_cross_entropy` for logits [N, H, W] or [N, 1, H, W] and a float target
    [N, H, W]: l = max(x, 0) - x t + log1p(exp(-|x|)), every pixel valid, loss = the mean of l over S."""
    return _ohem_bce(logits, target, keep_ratio, min_kept, thresh)[0]


_LOVASZ_STATS = ("n_valid", "n_classes", "fg_counts")


class _LovaszSoftmax(torch.autograd.Function):
    """ce_weight * pixel-wise cross-entropy + lovasz_weight * Lovasz-Softmax (csrc/kernels/lovasz.hip): logits read
    in place, the gradient in their strides; returns the loss and the three device statistics."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, classes, per_image, ce_weight, lovasz_weight):
        be, x, labels, _ = _pixel_inputs(logits, labels, None)
        loss, lse, g, coef, den, st = be.lovasz_softmax_fwd(x, labels, ignore_index, classes, per_image, ce_weight,
                                                            lovasz_weight)
        ctx.save_for_backward(x, labels, lse, g, coef, den)
        ctx.args, ctx.in_dtype = (ignore_index, per_image, ce_weight, lovasz_weight), logits.dtype
        stats = tuple(st[n] for n in _LOVASZ_STATS)
        ctx.mark_non_differentiable(*stats)
        return (loss,) + stats

    @staticmethod
    def backward(ctx, go, *_):
        x, labels, lse, g, coef, den = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        d = be.lovasz_softmax_bwd(x, labels, lse, g, coef, den, go.reshape(1).to(be.dt).contiguous(), *ctx.args)
        return (d.to(ctx.in_dtype),) + (None,) * 6


class _LovaszHinge(torch.autograd.Function):
    """bce_weight * BCE-with-logits + lovasz_weight * Lovasz hinge: contiguous logits and float targets [N, ...]."""

    @staticmethod
    def forward(ctx, logits, target, per_image, bce_weight, lovasz_weight):
        be = _be(logits.device, logits.dtype)
        x = logits.contiguous().to(be.dt)
        target = target.contiguous().to(be.dt)
        loss, g, coef, st = be.lovasz_hinge_fwd(x, target, per_image, bce_weight, lovasz_weight)
        ctx.save_for_backward(x, target, g, coef)
        ctx.args, ctx.in_dtype = (per_image, bce_weight, lovasz_weight), logits.dtype
        stats = tuple(st[n] for n in _LOVASZ_STATS)
        ctx.mark_non_differentiable(*stats)
        return (loss,) + stats

    @staticmethod
    def backward(ctx, go, *_):
        x, target, g, coef = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        d = be.lovasz_hinge_bwd(x, target, g, coef, go.reshape(1).to(be.dt).contiguous(), *ctx.args)
        return d.view(x.shape).to(ctx.in_dtype), None, None, None, None


def _check_lovasz_args(w0, w1, names, classes="present"):
    for v, n in ((w0, names[0]), (w1, names[1])):
        if not math.isfinite(v) or v < 0:
            raise ValueError(f"{n} must be finite and >= 0, got {v}")
    if w0 == 0 and w1 == 0:
        raise ValueError(f"{names[0]} and {names[1]} must not both be 0")
    if classes not in ("present", "all"):
        raise ValueError(f"classes must be 'present' or 'all', got {classes!r}")


def _lovasz_softmax(logits, labels, ignore_index, classes, per_image, ce_weight, lovasz_weight):
    ce_weight, lovasz_weight = float(ce_weight), float(lovasz_weight)
    _check_lovasz_args(ce_weight, lovasz_weight, ("ce_weight", "lovasz_weight"), classes)
    if logits.dim() != 4:
        raise ValueError(f"the Lovasz-Softmax loss takes [N, K, H, W] logits, got {tuple(logits.shape)}")
    _check_pixel_args(logits, labels)
    if lovasz_weight == 0:
        loss = _PixelCE.apply(logits, labels, None, int(ignore_index))
        return (loss if ce_weight == 1 else loss * ce_weight), None
    out = _LovaszSoftmax.apply(logits, labels, int(ignore_index), classes, bool(per_image), ce_weight, lovasz_weight)
    return out[0], dict(zip(_LOVASZ_STATS, out[1:]))


def _lovasz_hinge(logits, target, per_image, bce_weight, lovasz_weight):
    bce_weight, lovasz_weight = float(bce_weight), float(lovasz_weight)
    _check_lovasz_args(bce_weight, lovasz_weight, ("bce_weight", "lovasz_weight"))
    if logits.dim() == target.dim() + 1 and logits.shape[1] == 1:
        logits = logits.squeeze(1)
    if target.dim() < 2 or logits.shape != target.shape or not target.is_floating_point():
        raise ValueError(f"the Lovasz hinge loss takes logits [N, H, W] or [N, 1, H, W] and a float target [N, H, W], "
                         f"got {tuple(logits.shape)} and {target.dtype} {tuple(target.shape)}")
    if lovasz_weight == 0:
        loss = _BCE.apply(logits, target)
        return (loss if bce_weight == 1 else loss * bce_weight), None
    out = _LovaszHinge.apply(logits, target, bool(per_image), bce_weight, lovasz_weight)
    return out[0], dict(zip(_LOVASZ_STATS, out[1:]))


def lovasz_softmax(logits, labels, ignore_index=-100, classes="present", per_image=False):
    """The Lovasz-Softmax loss (Berman et al., CVPR 2018), the Lovasz extension of the Jaccard loss, for
    [N, K, H, W] logits and int64 [N, H, W] labels.  A segment is the set of pixels ranked together: one per class
    over the batch, or with ``per_image`` one per (sample, class).  A pixel is valid as in :func:`cross_entropy`
    (neither ``ignore_index`` nor outside [0, K)); invalid pixels get no rank, no count and an exact zero gradient.
    With p the softmax, fg = [y = c] and e = |fg - p_c|, a segment's valid pixels are ranked by e descending, equal
    e by ascending pixel index (n, h, w) -- a stable sort; -0 counts as +0, a NaN ranks first.  With G the segment's
    fg count, i a pixel's 0-based rank, F the fg pixels strictly before it, R = G - F and U = G + i - F, the Jaccard
    gradient is g = 1 / U (fg), R / (U (U + 1)) (bg), 1 where U = 0 (an absent class) -- J_i - J_{i-1} of the paper,
    formed in fp64 from the integers -- and the segment's loss is sum e g.  ``classes="present"`` averages the
    segments with G > 0, ``"all"`` every class; ``per_image`` averages over the samples each one's mean over its
    counted classes (0 for a sample without one).  Nothing to count: loss 0, zero gradient.  The gradient goes
    through e with g held constant.  On the GPU the ranking is a segmented stable radix sort
    (csrc/kernels/lovasz.hip): no host synchronisation, the same bits on every run."""
    return _lovasz_softmax(logits, labels, ignore_index, classes, per_image, 0.0, 1.0)[0]


def lovasz_hinge(logits, target, per_image=True):
    """The binary Lovasz hinge loss for logits [N, H, W] or [N, 1, H, W] and a float target [N, H, W]: fg =
    [t > 0.5], e = 1 - x (2 fg - 1), every pixel valid, one class; ranking and g as :func:`lovasz_softmax`, the
    segment's loss is sum max(e, 0) g and dx = -(2 fg - 1) g [e > 0].  ``per_image`` (the paper's default) ranks
    each sample on its own and averages the samples."""
    return _lovasz_hinge(logits, target, per_image, 0.0, 1.0)[0]


def ce_lovasz_loss(logits, labels, ignore_index=-100, classes="present", per_image=False, ce_weight=1.0,
                   lovasz_weight=1.0):
    """``ce_weight * CE + lovasz_weight * Lovasz-Softmax`` with CE the plain unweighted :func:`cross_entropy` over
    the valid pixels.  On the GPU the CE sum rides in the error pass and its gradient in the one backward pass;
    ``lovasz_weight=0`` is :func:`cross_entropy` itself (the plain kernels), ``ce_weight=0`` the Lovasz term alone."""
    return _lovasz_softmax(logits, labels, ignore_index, classes, per_image, ce_weight, lovasz_weight)[0]


def bce_lovasz_loss(logits, target, per_image=True, bce_weight=1.0, lovasz_weight=1.0):
    """``bce_weight * BCE + lovasz_weight * Lovasz hinge``; ``lovasz_weight=0`` is :func:`bce_with_logits` itself."""
    return _lovasz_hinge(logits, target, per_image, bce_weight, lovasz_weight)[0]


class CELovaszLoss(nn.Module):
    """:func:`ce_lovasz_loss`; ``last_stats`` holds the latest forward's device tensors ``n_valid``, ``n_classes``
    (counted segments) and ``fg_counts`` (int32), which the library itself never reads (None at
    ``lovasz_weight=0``)."""

    def __init__(self, ignore_index=-100, classes="present", per_image=False, ce_weight=1.0, lovasz_weight=1.0):
        super().__init__()
        _check_lovasz_args(float(ce_weight), float(lovasz_weight), ("ce_weight", "lovasz_weight"), classes)
        self.ignore_index, self.classes, self.per_image = ignore_index, classes, per_image
        self.ce_weight, self.lovasz_weight = ce_weight, lovasz_weight
        self.last_stats = None

    def forward(self, logits, labels):
        loss, self.last_stats = _lovasz_softmax(logits, labels, self.ignore_index, self.classes, self.per_image,
                                                self.ce_weight, self.lovasz_weight)
        return loss


class LovaszSoftmaxLoss(CELovaszLoss):
    """:func:`lovasz_softmax`; ``last_stats`` as :class:`CELovaszLoss`."""

    def __init__(self, ignore_index=-100, classes="present", per_image=False):
        super().__init__(ignore_index, classes, per_image, 0.0, 1.0)


class BCELovaszLoss(nn.Module):
    """:func:`bce_lovasz_loss`; ``last_stats`` as :class:`CELovaszLoss`."""

    def __init__(self, per_image=True, bce_weight=1.0, lovasz_weight=1.0):
        super().__init__()
        _check_lovasz_args(float(bce_weight), float(lovasz_weight), ("bce_weight", "lovasz_weight"))
        self.per_image, self.bce_weight, self.lovasz_weight = per_image, bce_weight, lovasz_weight
        self.last_stats = None

    def forward(self, logits, target):
        loss, self.last_stats = _lovasz_hinge(logits, target, self.per_image, self.bce_weight, self.lovasz_weight)
        return loss


class LovaszHingeLoss(BCELovaszLoss):
    """:func:`lovasz_hinge`; ``last_stats`` as :class:`CELovaszLoss`."""

    def __init__(self, per_image=True):
        super().__init__(per_image, 0.0, 1.0)


def edt_squared(mask):
    """Exact squared Euclidean distance transform: bool ``mask`` [..., H, W] -> int32 of that shape, the squared
    distance ``dy^2 + dx^2`` of every pixel to the nearest True pixel of its plane (0 on the True pixels),
    ``INT32_MAX`` where the plane has none.  On the GPU a separable integer transform (csrc/kernels/edt.hip: H <= 4096,
    W <= 16384), no host synchronisation."""
    if mask.dim() < 2 or mask.dtype != torch.bool:
        raise ValueError(f"edt_squared takes a bool mask [..., H, W], got {mask.dtype} {tuple(mask.shape)}")
    be = _be(mask.device)
    return be.edt_squared(mask.reshape(-1, *mask.shape[-2:])).view(mask.shape)


def signed_distance_map(labels, num_classes=None, ignore_index=-100):
    """The signed distance maps of the boundary loss (Kervadec et al., MIDL 2019, ``one_hot2dist``).  int64 labels
    [N, H, W] with ``num_classes`` K -> fp32 [N, K, H, W]; a float target [N, H, W] (fg = t > 0.5) -> fp32 [N, H, W].
    With G the pixels of the class (ignored and out-of-range pixels are in no G): +sqrt(d2) to the nearest pixel of G
    outside it, 1 - sqrt(d2) to the nearest pixel outside G inside it (inner border 0, interior negative), 0 for a
    class that is absent from the sample or fills it.  The distances are exact integers, the root is rounded once."""
    if labels.dim() != 3 or not (labels.dtype == torch.int64 or labels.is_floating_point()):
        raise ValueError(f"signed_distance_map takes int64 labels or a float target [N, H, W], got {labels.dtype} "
                         f"{tuple(labels.shape)}")
    be = _be(labels.device)
    if labels.dtype != torch.int64:
        return be.signed_distance(labels.to(torch.float32).contiguous())
    if num_classes is None or not 1 <= int(num_classes) <= 256:
        raise ValueError(f"int64 labels need num_classes in 1..256, got {num_classes}")
    return be.signed_distance(labels.contiguous(), int(num_classes), int(ignore_index))


class _BoundarySoftmax(torch.autograd.Function):
    """ce_weight * pixel-wise cross-entropy + boundary_weight * boundary loss (csrc/kernels/boundary.hip): logits
    read in place, the gradient in their strides; ``bw`` is a float or a one-element device tensor that both passes
    read in place."""

    @staticmethod
    def forward(ctx, logits, labels, phi, ignore_index, include_background, ce_weight, bw):
        be, x, labels, _ = _pixel_inputs(logits, labels, None)
        loss, lse, den = be.boundary_softmax_fwd(x, labels, phi, ignore_index, include_background, ce_weight, bw)
        ctx.save_for_backward(x, labels, phi, lse, den)
        ctx.args, ctx.in_dtype = (ignore_index, include_background, ce_weight, bw), logits.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        x, labels, phi, lse, den = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        d = be.boundary_softmax_bwd(x, labels, phi, lse, den, go.reshape(1).to(be.dt).contiguous(), *ctx.args)
        return (d.to(ctx.in_dtype),) + (None,) * 6


class _BoundarySigmoid(torch.autograd.Function):
    """bce_weight * BCE-with-logits + boundary_weight * mean(sigmoid(x) phi): contiguous logits, float targets."""

    @staticmethod
    def forward(ctx, logits, target, phi, bce_weight, bw):
        be = _be(logits.device, logits.dtype)
        x = logits.contiguous().to(be.dt)
        target = target.contiguous().to(be.dt)
        loss = be.boundary_sigmoid_fwd(x, target, phi, bce_weight, bw)
        ctx.save_for_backward(x, target, phi)
        ctx.args, ctx.in_dtype = (bce_weight, bw), logits.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        x, target, phi = ctx.saved_tensors
        be = _be(x.device, x.dtype)
        d = be.boundary_sigmoid_bwd(x, target, phi, go.reshape(1).to(be.dt).contiguous(), *ctx.args)
        return d.view(x.shape).to(ctx.in_dtype), None, None, None, None


def _check_boundary_weights(plain, bw, names, device=None):
    """-> (plain weight, boundary weight: a float or a one-element fp32 tensor on ``device``)."""
    plain = float(plain)
    if not math.isfinite(plain) or plain < 0:
        raise ValueError(f"{names[0]} must be finite and >= 0, got {plain}")
    if torch.is_tensor(bw):
        if bw.numel() != 1 or bw.dtype != torch.float32 or (device is not None and bw.device != device):
            raise ValueError(f"a tensor {names[1]} is one fp32 element on the device of the logits")
        return plain, bw
    bw = float(bw)
    if not math.isfinite(bw) or bw < 0:
        raise ValueError(f"{names[1]} must be finite and >= 0, got {bw}")
    if plain == 0 and bw == 0:
        raise ValueError(f"{names[0]} and {names[1]} must not both be 0")
    return plain, bw


def _boundary(logits, target, ignore_index, include_background, dist, plain_weight, boundary_weight, names):
    plain_weight, bw = _check_boundary_weights(plain_weight, boundary_weight, names, logits.device)
    be = _be(logits.device, logits.dtype)
    if target.dtype == torch.int64:
        if logits.dim() != 4:
            raise ValueError(f"the boundary loss takes [N, K, H, W] logits with int64 labels, got {tuple(logits.shape)}")
        _check_pixel_args(logits, target)
        if not include_background and logits.shape[1] < 2:
            raise ValueError("include_background=False needs at least two classes")
        if not torch.is_tensor(bw) and bw == 0:
            loss = _PixelCE.apply(logits, target, None, int(ignore_index))
            return loss if plain_weight == 1 else loss * plain_weight
        shape = tuple(logits.shape)
        if dist is None:
            dist = be.signed_distance(target.contiguous(), shape[1], int(ignore_index))
        elif tuple(dist.shape) != shape:
            raise ValueError(f"dist must be the signed_distance_map of the labels, {shape}, got {tuple(dist.shape)}")
        return _BoundarySoftmax.apply(logits, target, dist.to(be.dt).contiguous(), int(ignore_index),
                                      bool(include_background), plain_weight, bw)
    if logits.dim() == target.dim() + 1 and logits.shape[1] == 1:
        logits = logits.squeeze(1)
    if target.dim() != 3 or logits.shape != target.shape or not target.is_floating_point():
        raise ValueError(f"the binary boundary loss takes logits [N, H, W] or [N, 1, H, W] and a float target "
                         f"[N, H, W], got {tuple(logits.shape)} and {target.dtype} {tuple(target.shape)}")
    if not torch.is_tensor(bw) and bw == 0:
        loss = _BCE.apply(logits, target)
        return loss if plain_weight == 1 else loss * plain_weight
    if dist is None:
        dist = be.signed_distance(target.to(torch.float32).contiguous())
    elif dist.shape != target.shape:
        raise ValueError(f"dist must be the signed_distance_map of the target, {tuple(target.shape)}, got "
                         f"{tuple(dist.shape)}")
    return _BoundarySigmoid.apply(logits, target, dist.to(be.dt).contiguous(), plain_weight, bw)


def boundary_loss(logits, target, ignore_index=-100, include_background=True, dist=None):
    """The boundary (surface) loss of Kervadec et al. (MIDL 2019).  int64 ``target`` [N, H, W] with [N, K, H, W]
    logits: B = sum over the valid pixels and the classes C of softmax_c * phi_c / (n_valid |C|), phi =
    :func:`signed_distance_map` of the labels, C every class or 1..K-1 without the background, a pixel valid as in
    :func:`cross_entropy`; nothing valid: loss 0, zero gradient; invalid pixels get an exact zero gradient.  A float
    ``target`` [N, H, W] with logits [N, H, W] or [N, 1, H, W]: B = mean(sigmoid(x) * phi) with phi the map of
    t > 0.5.  ``dist`` takes a precomputed :func:`signed_distance_map` (static masks pay for the transform once);
    without it the map is computed on the device in the same stream (csrc/kernels/edt.hip), so the loss needs no host
    synchronisation and captures into a graph with its labels."""
    return _boundary(logits, target, ignore_index, include_background, dist, 0.0, 1.0, ("ce_weight", "boundary_weight"))


def ce_boundary_loss(logits, labels, ignore_index=-100, include_background=True, dist=None, ce_weight=1.0,
                     boundary_weight=0.01):
    """``ce_weight * CE + boundary_weight * boundary_loss`` with CE the plain unweighted :func:`cross_entropy` over
    the valid pixels, in one fused forward and one backward pass.  ``boundary_weight`` is a float or a one-element fp32
    tensor on the device, which the kernels read (a rebalancing schedule can then move under graph replay); a float 0
    is :func:`cross_entropy` itself (the plain kernels), a tensor always takes the fused path."""
    return _boundary(logits, labels, ignore_index, include_background, dist, ce_weight, boundary_weight,
                     ("ce_weight", "boundary_weight"))


def bce_boundary_loss(logits, target, dist=None, bce_weight=1.0, boundary_weight=0.01):
    """``bce_weight * BCE + boundary_weight * boundary_loss`` for a float target; ``boundary_weight`` as
    :func:`ce_boundary_loss`, a float 0 is :func:`bce_with_logits` itself."""
    if not target.is_floating_point():
        raise ValueError(f"bce_boundary_loss takes a float target, got {target.dtype}")
    return _boundary(logits, target, -100, True, dist, bce_weight, boundary_weight, ("bce_weight", "boundary_weight"))


class CEBoundaryLoss(nn.Module):
    """:func:`ce_boundary_loss`.  ``boundary_weight`` may be replaced by a one-element device tensor at any time."""

    def __init__(self, ignore_index=-100, include_background=True, ce_weight=1.0, boundary_weight=0.01):
        super().__init__()
        _check_boundary_weights(ce_weight, boundary_weight, ("ce_weight", "boundary_weight"))
        self.ignore_index, self.include_background = ignore_index, include_background
        self.ce_weight, self.boundary_weight = ce_weight, boundary_weight

    def forward(self, logits, labels, dist=None):
        return ce_boundary_loss(logits, labels, self.ignore_index, self.include_background, dist, self.ce_weight,
                                self.boundary_weight)


class BCEBoundaryLoss(nn.Module):
    """:func:`bce_boundary_loss`; ``boundary_weight`` as :class:`CEBoundaryLoss`."""

    def __init__(self, bce_weight=1.0, boundary_weight=0.01):
        super().__init__()
        _check_boundary_weights(bce_weight, boundary_weight, ("bce_weight", "boundary_weight"))
        self.bce_weight, self.boundary_weight = bce_weight, boundary_weight

    def forward(self, logits, target, dist=None):
        return bce_boundary_loss(logits, target, dist, self.bce_weight, self.boundary_weight)


class BoundaryLoss(nn.Module):
    """:func:`boundary_loss`, either form by the target's dtype."""

    def __init__(self, ignore_index=-100, include_background=True):
        super().__init__()
        self.ignore_index, self.include_background = ignore_index, include_background

    def forward(self, logits, target, dist=None):
        return boundary_loss(logits, target, self.ignore_index, self.include_background, dist)


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


class OHEMCrossEntropyLoss(nn.Module):
    """:func:`ohem_cross_entropy`; ``last_stats`` holds the latest forward's device tensors ``cut`` (fp32), ``k``,
    ``n_valid`` and ``n_selected`` (int32), one element each, which the library itself never reads."""

    def __init__(self, weight=None, ignore_index=-100, keep_ratio=0.25, min_kept=1, thresh=None):
        super().__init__()
        self.register_buffer("weight", weight)
        self.ignore_index = ignore_index
        self.keep_ratio, self.min_kept, self.thresh = _check_ohem_args(keep_ratio, min_kept, thresh)
        self.last_stats = None

    def forward(self, logits, labels):
        loss, self.last_stats = _ohem_ce(logits, labels, self.weight, self.ignore_index, self.keep_ratio,
                                         self.min_kept, self.thresh)
        return loss


class OHEMBCEWithLogitsLoss(nn.Module):
    """:func:`ohem_bce_with_logits`; ``last_stats`` as :class:`OHEMCrossEntropyLoss`."""

    def __init__(self, keep_ratio=0.25, min_kept=1, thresh=None):
        super().__init__()
        self.keep_ratio, self.min_kept, self.thresh = _check_ohem_args(keep_ratio, min_kept, thresh)
        self.last_stats = None

    def forward(self, logits, target):
        loss, self.last_stats = _ohem_bce(logits, target, self.keep_ratio, self.min_kept, self.thresh)
        return loss


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
def surface_distances(logits, target, ignore_index=-100, percentile=95.0):
    """Surface-distance metrics per sample and class -> (``metrics`` fp32 [N, K, 3], ``counts`` int64 [N, K, 2]).
    int64 ``target`` [N, H, W] with logits [N, K, H, W] (either pixel layout, read in place): pred = argmax (ties to
    the lowest index), pixels whose label is ``ignore_index`` or outside [0, K) are in no class of either map.  A
    float ``target`` with logits [N, H, W] or [N, 1, H, W]: pred = x > 0, gt = t > 0.5, the one class the foreground.
    With P, G the 4-connected edge pixels of class c in pred and gt and D(A->B) the exact Euclidean distances of A's
    pixels to the nearest pixel of B: ``metrics`` = {max(max D(P->G), max D(G->P)) (Hausdorff), the maximum over both
    directions of the ``percentile``-th percentile by numpy's ``linear`` rule (HD95), (sum D(P->G) + sum D(G->P)) /
    (|P| + |G|) (ASSD)}, ``counts`` = {|P|, |G|}.  NaN where both sets are empty, +inf where exactly one is.  On the
    GPU csrc/kernels/surface.hip (H <= 4096, W <= 16384), no host synchronisation, the same bits on every run."""
    if not 0.0 < float(percentile) <= 100.0:   # (a NaN fails too)
        raise ValueError(f"surface_distances: percentile must lie in (0, 100], got {percentile}")
    if target.dtype == torch.int64:
        if logits.dim() != 4:
            raise ValueError(f"surface_distances takes [N, K, H, W] logits with int64 labels, got "
                             f"{tuple(logits.shape)}")
        _check_pixel_args(logits, target)
        be = _be(logits.device, logits.dtype)
        return be.surface_distances(_pixel_layout(logits.detach()).to(be.dt), target.contiguous(), int(ignore_index),
                                    float(percentile))
    x = logits.squeeze(1) if logits.dim() == 4 and logits.shape[1] == 1 else logits
    if x.dim() != 3 or not target.is_floating_point() or target.shape != x.shape:
        raise ValueError(f"the binary surface_distances takes logits [N, H, W] or [N, 1, H, W] and a float target "
                         f"[N, H, W], got {tuple(logits.shape)} and {target.dtype} {tuple(target.shape)}")
    be = _be(logits.device, logits.dtype)
    return be.surface_distances(x.detach().to(be.dt).contiguous(), target.to(be.dt).contiguous(), int(ignore_index),
                                float(percentile))


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
