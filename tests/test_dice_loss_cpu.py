"""Soft Dice losses on the CPU (reference backend, float64): ce_dice_loss / dice_loss / bce_dice_loss against
a composition of F.softmax / F.one_hot / F.cross_entropy and autograd written here (it does not call
RefBackend), the edge cases of the definition, a UNet(out_classes=3) engine step with ce+dice against torch
autograd, and the trainer's --loss flag."""
import copy
import glob
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from deeplearning_mpi_amd.models import UNet
from deeplearning_mpi_amd.ops import (BCEDiceLoss, BCEWithLogitsLoss, CEDiceLoss, CrossEntropyLoss, DiceLoss,
                                      bce_dice_loss, bce_with_logits, ce_dice_loss, cross_entropy, dice_loss)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 9, 11
TOL = 1e-10


def _keep(y, K, ignore_index):
    return (y != ignore_index) & (y >= 0) & (y < K)


def soft_dice(x, y, K, ignore_index=-100, smooth=1.0, include_background=True):
    """1 - mean over samples and classes of (2 I + smooth) / (P + T + smooth), over the kept pixels."""
    keep = _keep(y, K, ignore_index).unsqueeze(1)
    p = F.softmax(x, 1) * keep
    oh = F.one_hot(y.clamp(0, K - 1), K).permute(0, 3, 1, 2).to(x.dtype) * keep
    dice = (2 * (p * oh).sum((2, 3)) + smooth) / (p.sum((2, 3)) + oh.sum((2, 3)) + smooth)
    if not include_background:
        dice = dice[:, 1:]
    return 1 - dice.mean()


def composed(x, y, K, weight=None, ignore_index=-100, ce_weight=1.0, dice_weight=1.0, smooth=1.0,
             include_background=True):
    loss = dice_weight * soft_dice(x, y, K, ignore_index, smooth, include_background)
    if ce_weight != 0:
        yr = torch.where(_keep(y, K, ignore_index), y, torch.full_like(y, ignore_index))
        loss = loss + ce_weight * F.cross_entropy(x, yr, weight=weight, ignore_index=ignore_index)
    return loss


def composed_binary(x, t, bce_weight=1.0, dice_weight=1.0, smooth=1.0):
    p = torch.sigmoid(x).flatten(1)
    tf = t.flatten(1)
    dice = (2 * (p * tf).sum(1) + smooth) / (p.sum(1) + tf.sum(1) + smooth)
    loss = dice_weight * (1 - dice.mean())
    if bce_weight != 0:
        loss = loss + bce_weight * F.binary_cross_entropy_with_logits(x, t)
    return loss


def _logits(K, layout, g):
    base = torch.randn(N, H, W, K, generator=g, dtype=torch.float64)
    x = base.permute(0, 3, 1, 2)
    return x if layout == "nhwc_view" else x.contiguous()


def _labels(g, K, ignore_index=-100):
    y = torch.randint(K, (N, H, W), generator=g)
    y[0, :3] = ignore_index   # ignored rows
    y[1, 5, 7] = K + 3        # out of range: ignored as well
    return y


def _both(x, ours, ref):
    """(our loss, our gradient, reference loss, reference gradient) on x and a detached copy."""
    x = x.requires_grad_(True)
    la = ours(x)
    (ga,) = torch.autograd.grad(la, x)
    xr = x.detach().clone().requires_grad_(True)
    lr = ref(xr)
    (gr,) = torch.autograd.grad(lr, xr)
    return la, ga, lr, gr


@pytest.mark.parametrize("smooth", [1.0, 1e-5])
@pytest.mark.parametrize("include_background", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_ce_dice_and_dice_match_composition_fp64(K, layout, weighted, include_background, smooth):
    g = torch.Generator().manual_seed(K)
    x = _logits(K, layout, g)
    y = _labels(g, K)
    w = torch.rand(K, generator=g, dtype=torch.float64) + 0.5 if weighted else None
    kw = dict(smooth=smooth, include_background=include_background)
    la, ga, lr, gr = _both(x, lambda t: ce_dice_loss(t, y, weight=w, ce_weight=0.7, dice_weight=1.3, **kw),
                           lambda t: composed(t, y, K, w, -100, 0.7, 1.3, **kw))
    assert abs(la.item() - lr.item()) < TOL
    assert (ga - gr).abs().max().item() < TOL
    assert ga.stride() == x.stride() and ga.dtype == torch.float64
    assert (ga[0, :, :3] == 0).all() and (ga[1, :, 5, 7] == 0).all()   # exact zeros at ignored pixels
    if not weighted:
        la, ga, lr, gr = _both(x.detach(), lambda t: dice_loss(t, y, **kw),
                               lambda t: composed(t, y, K, None, -100, 0.0, 1.0, **kw))
        assert abs(la.item() - lr.item()) < TOL
        assert (ga - gr).abs().max().item() < TOL
        assert ga.stride() == x.stride()
        assert (ga[0, :, :3] == 0).all() and (ga[1, :, 5, 7] == 0).all()


@pytest.mark.parametrize("K", [2, 5])
def test_second_ignore_index(K):
    g = torch.Generator().manual_seed(10 + K)
    x = _logits(K, "nhwc_view", g)
    y = _labels(g, K, ignore_index=255)
    y[1, 0, :4] = -100   # with ignore_index 255 a -100 is merely out of range: ignored as well
    la, ga, lr, gr = _both(x, lambda t: ce_dice_loss(t, y, ignore_index=255), lambda t: composed(t, y, K, None, 255))
    assert abs(la.item() - lr.item()) < TOL and (ga - gr).abs().max().item() < TOL
    assert (ga[0, :, :3] == 0).all() and (ga[1, :, 5, 7] == 0).all() and (ga[1, :, 0, :4] == 0).all()
    la, ga, lr, gr = _both(x.detach(), lambda t: DiceLoss(ignore_index=255)(t, y),
                           lambda t: composed(t, y, K, None, 255, 0.0))
    assert abs(la.item() - lr.item()) < TOL and (ga - gr).abs().max().item() < TOL


@pytest.mark.parametrize("smooth", [1.0, 1e-5])
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("shape", ["nhw", "n1hw"])
def test_bce_dice_matches_composition_fp64(shape, soft, smooth):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, W, generator=g, dtype=torch.float64) * 2
    t = torch.rand(N, H, W, generator=g, dtype=torch.float64)
    if not soft:
        t = (t > 0.6).double()
    xin = x.unsqueeze(1) if shape == "n1hw" else x
    view = (lambda v: v.squeeze(1)) if shape == "n1hw" else (lambda v: v)
    la, ga, lr, gr = _both(xin.clone(), lambda v: bce_dice_loss(v, t, 0.8, 1.2, smooth),
                           lambda v: composed_binary(view(v), t, 0.8, 1.2, smooth))
    assert abs(la.item() - lr.item()) < TOL and (ga - gr).abs().max().item() < TOL
    assert ga.shape == xin.shape
    la, ga, lr, gr = _both(xin.clone(), lambda v: dice_loss(v, t, smooth=smooth),
                           lambda v: composed_binary(view(v), t, 0.0, 1.0, smooth))
    assert abs(la.item() - lr.item()) < TOL and (ga - gr).abs().max().item() < TOL
    m = BCEDiceLoss(0.8, 1.2, smooth)
    assert abs(m(xin, t).item() - composed_binary(x, t, 0.8, 1.2, smooth).item()) < TOL


@pytest.mark.parametrize("K", [2, 3])
def test_all_ignored_batch(K):
    g = torch.Generator().manual_seed(1)
    x = _logits(K, "nhwc_view", g).requires_grad_(True)
    y = torch.full((N, H, W), -100, dtype=torch.int64)
    ld = dice_loss(x, y)
    (gd,) = torch.autograd.grad(ld, x)
    assert ld.item() == 0.0 and (gd == 0).all()          # every dice is smooth / smooth = 1 exactly
    lc = ce_dice_loss(x, y)
    (gc,) = torch.autograd.grad(lc, x)
    assert torch.isnan(lc) and (gc == 0).all()           # the cross-entropy's rule: 0 / 0, zero gradient
    # one sample all ignored, the other not: the empty sample contributes dice = 1 and no gradient
    y2 = _labels(g, K)
    y2[0] = -100
    la, ga, lr, gr = _both(x.detach(), lambda t: ce_dice_loss(t, y2), lambda t: composed(t, y2, K))
    assert abs(la.item() - lr.item()) < TOL and (ga - gr).abs().max().item() < TOL
    assert (ga[0] == 0).all() and ga[1].abs().max() > 0


def test_absent_class_and_never_likely_class():
    """Sample 1: class 3 absent from the labels (its dice falls with any probability it gets), class 2 at
    -50 everywhere while it is labelled (p ~ 0: dice ~ smooth / (T + smooth))."""
    K = 4
    g = torch.Generator().manual_seed(3)
    x = _logits(K, "nchw", g)
    x[1, 2] = -50.0
    y = _labels(g, K)
    y[1][y[1] == 3] = 0
    for bg in (True, False):
        la, ga, lr, gr = _both(x.clone(), lambda t: ce_dice_loss(t, y, include_background=bg),
                               lambda t: composed(t, y, K, include_background=bg))
        assert abs(la.item() - lr.item()) < TOL and (ga - gr).abs().max().item() < TOL
    assert torch.isfinite(ga).all() and ga[1, 3].abs().max() > 0


def test_zero_dice_weight_is_the_existing_loss_bit_for_bit():
    g = torch.Generator().manual_seed(7)
    K = 3
    x = _logits(K, "nhwc_view", g).requires_grad_(True)
    y = _labels(g, K)
    w = torch.rand(K, generator=g, dtype=torch.float64) + 0.5
    l1, l2 = ce_dice_loss(x, y, weight=w, dice_weight=0.0), cross_entropy(x, y, weight=w)
    (g1,), (g2,) = torch.autograd.grad(l1, x), torch.autograd.grad(l2, x)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    xb = torch.randn(N, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    t = (torch.rand(N, H, W, generator=g) > 0.5).double()
    l1, l2 = bce_dice_loss(xb, t, dice_weight=0.0), bce_with_logits(xb, t)
    (g1,), (g2,) = torch.autograd.grad(l1, xb), torch.autograd.grad(l2, xb)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_argument_errors():
    x = torch.randn(2, 3, 4, 5, dtype=torch.float64)
    y = torch.randint(3, (2, 4, 5))
    t = torch.rand(2, 4, 5, dtype=torch.float64)
    for smooth in (0.0, -1.0):
        with pytest.raises(ValueError):
            ce_dice_loss(x, y, smooth=smooth)
        with pytest.raises(ValueError):
            dice_loss(x, y, smooth=smooth)
        with pytest.raises(ValueError):
            bce_dice_loss(x[:, 0], t, smooth=smooth)
    with pytest.raises(ValueError):
        ce_dice_loss(x, y, ce_weight=0.0, dice_weight=0.0)
    with pytest.raises(ValueError):
        bce_dice_loss(x[:, 0], t, bce_weight=0.0, dice_weight=0.0)
    with pytest.raises(ValueError):
        ce_dice_loss(x, y, dice_weight=-1.0)
    with pytest.raises(ValueError):
        ce_dice_loss(x, y, ce_weight=float("inf"))
    with pytest.raises(ValueError):
        ce_dice_loss(x, y.float())                 # label dtype
    with pytest.raises(ValueError):
        ce_dice_loss(x, y[:, :3])                  # label shape
    with pytest.raises(ValueError):
        dice_loss(x, y.to(torch.int32))            # neither int64 class indices nor a float target
    with pytest.raises(ValueError):
        bce_dice_loss(x, t)                        # [N, 3, H, W] logits against [N, H, W]
    with pytest.raises(ValueError):
        ce_dice_loss(x, y, weight=torch.ones(4, dtype=torch.float64))
    # include_background=False with two classes: the one foreground class
    x2 = x[:, :2].clone()
    y2 = y.clamp_max(1)
    la, ga, lr, gr = _both(x2, lambda v: CEDiceLoss(include_background=False)(v, y2),
                           lambda v: composed(v, y2, 2, include_background=False))
    assert abs(la.item() - lr.item()) < TOL and (ga - gr).abs().max().item() < TOL


def _err(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def test_unet_ce_dice_train_step_matches_torch():
    """UNet(out_classes=3) in float64 at 16x16: engine + ce_dice_loss against eager autograd of the composition."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, 16, 16, generator=g, dtype=torch.float64)
    y = torch.randint(3, (4, 16, 16), generator=g)
    y[0, :2] = -100
    torch.manual_seed(0)
    m1 = UNet(out_classes=3).double()
    m3 = copy.deepcopy(m1)
    m1.train()
    m3.train()
    o1 = m1(x)
    l1 = ce_dice_loss(o1, y)
    l1.backward()
    o3 = m3.forward_torch(x)
    l3 = composed(o3, y, 3)
    l3.backward()
    assert _err(o1.detach(), o3.detach()) < 1e-9 and abs(l1.item() - l3.item()) < 1e-9
    checked = 0
    for (n, p1), (_, p3) in zip(m1.named_parameters(), m3.named_parameters()):
        if (n.endswith("bias") and "double_conv.double_conv" in n) or p3.grad.abs().max() == 0:
            continue   # conv bias before a training BN: gradient exactly zero
        assert _err(p1.grad, p3.grad) < 1e-9, (n, _err(p1.grad, p3.grad))
        checked += 1
    assert checked > 10


def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("flags", [["--num_classes", "3", "--loss", "ce+dice"],
                                   ["--num_classes", "1", "--loss", "dice"]])
def test_trainer_loss_flag_on_cpu(tmp_path, flags):
    logs = tmp_path / "logs"
    r = _run([sys.executable, "pytorch/unet/train.py", "--device", "cpu", "--backend", "gloo", "--synthetic",
              "--image_size", "32", "--num_epochs", "1", "--workers", "0", "--batch_size", "2", "--synthetic_size", "6",
              "--eval_every", "1", "--log_dir", str(logs), "--model_dir", str(tmp_path)] + flags)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    (log,) = glob.glob(str(logs / "training_log_*.log"))
    line = [ln for ln in open(log).read().splitlines() if "| Loss:" in ln][0]
    loss = float(line.split("Loss:")[1].split("|")[0])
    assert loss == loss and 0.0 < loss < 1e3, line   # finite; random weights leave both terms well above 0


def test_default_arguments_build_todays_criteria():
    from deeplearning_mpi_amd.apps import segmentation as seg

    p = seg.build_argparser()
    a = p.parse_args([])
    assert (a.loss, a.dice_weight, a.dice_smooth, a.dice_background) == ("ce", 1.0, 1.0, 1)
    assert type(seg.build_criterion(a)) is BCEWithLogitsLoss
    c = seg.build_criterion(p.parse_args(["--num_classes", "3", "--ignore_index", "7"]))
    assert type(c) is CrossEntropyLoss and c.ignore_index == 7 and c.weight is None
    c = seg.build_criterion(p.parse_args(["--num_classes", "3", "--loss", "ce+dice", "--dice_weight", "0.5",
                                          "--dice_smooth", "2", "--dice_background", "0", "--ignore_index", "7"]))
    assert type(c) is CEDiceLoss and (c.ce_weight, c.dice_weight, c.smooth, c.include_background, c.ignore_index) == \
        (1.0, 0.5, 2.0, False, 7)
    c = seg.build_criterion(p.parse_args(["--num_classes", "3", "--loss", "dice", "--ignore_index", "7"]))
    assert type(c) is DiceLoss and c.ignore_index == 7 and c.include_background is True
    assert type(seg.build_criterion(p.parse_args(["--loss", "ce+dice"]))) is BCEDiceLoss
    assert type(seg.build_criterion(p.parse_args(["--loss", "dice"]))) is DiceLoss
