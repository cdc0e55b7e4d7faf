"""Soft Dice fused into the pixel cross-entropy / BCE kernels (csrc/kernels/seg_dice.hip) against the fp64
composition of the fp32 logits (F.softmax / F.one_hot / F.cross_entropy and autograd): every kernel path
(K in registers, vector access, LDS tiles, the generic path), both layouts, class weights, the per-sample
grid, several blocks per sample, a misaligned buffer, the binary form, the edge cases of the definition,
run-to-run determinism, and a K-class UNet step: kernels launched, hipGraph replay, training, the trainer.

Tolerances are those of tests/test_pixel_ce_gpu.py (__expf / __logf arithmetic): loss |d| < 1e-4, gradient
relative L2 < 1e-4."""
import copy
import glob
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from deeplearning_mpi_amd.ops import (backward, bce_dice_loss, bce_with_logits, ce_dice_loss, cross_entropy,
                                      dice_loss)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 17, 23   # 391 pixels per sample: no multiple of 64 or 256, tail lanes and partial tiles live


def _keep(y, K, ignore_index=-100):
    return (y != ignore_index) & (y >= 0) & (y < K)


def composed(x, y, K, weight=None, ce_weight=1.0, dice_weight=1.0, smooth=1.0, include_background=True):
    keep = _keep(y, K).unsqueeze(1)
    p = F.softmax(x, 1) * keep
    oh = F.one_hot(y.clamp(0, K - 1), K).permute(0, 3, 1, 2).to(x.dtype) * keep
    dice = (2 * (p * oh).sum((2, 3)) + smooth) / (p.sum((2, 3)) + oh.sum((2, 3)) + smooth)
    if not include_background:
        dice = dice[:, 1:]
    loss = dice_weight * (1 - dice.mean())
    if ce_weight != 0:
        yr = torch.where(keep.squeeze(1), y, torch.full_like(y, -100))
        loss = loss + ce_weight * F.cross_entropy(x, yr, weight=weight)
    return loss


def composed_binary(x, t, bce_weight=1.0, dice_weight=1.0, smooth=1.0):
    p, tf = torch.sigmoid(x).flatten(1), t.flatten(1)
    dice = (2 * (p * tf).sum(1) + smooth) / (p.sum(1) + tf.sum(1) + smooth)
    loss = dice_weight * (1 - dice.mean())
    if bce_weight != 0:
        loss = loss + bce_weight * F.binary_cross_entropy_with_logits(x, t)
    return loss


def _logits(K, layout, seed, shape=(N, H, W)):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(*shape, K, device=DEV, generator=g).permute(0, 3, 1, 2)
    return x if layout == "nhwc_view" else x.contiguous()


def _labels(K, seed, shape=(N, H, W)):
    g = torch.Generator(device=DEV).manual_seed(seed + 100)
    y = torch.randint(K, shape, device=DEV, generator=g)
    y[0, :3] = -100
    y[-1, 5, 7] = K + 3   # out of range: ignored as well
    return y


def _rel_l2(a, ref):
    a, ref = a.double().flatten(), ref.double().flatten()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _check(x, y, K, tag, weight=None, **kw):
    x = x.requires_grad_(True)
    loss = ce_dice_loss(x, y, weight=weight, **kw)
    (gx,) = torch.autograd.grad(loss, x)
    xr = x.detach().double().requires_grad_(True)
    lr = composed(xr, y, K, weight.double() if weight is not None else None, **kw)
    (gr,) = torch.autograd.grad(lr, xr)
    torch.cuda.synchronize()
    dl, dg = abs(loss.item() - lr.item()), _rel_l2(gx, gr)
    print(f"{tag}: loss |d| {dl:.3e}, grad rel L2 {dg:.3e}")
    assert dl < 1e-4
    assert dg < 1e-4
    assert gx.stride() == x.stride() and gx.dtype == torch.float32
    assert (gx[0, :, :3] == 0).all() and (gx[-1, :, 5, 7] == 0).all()   # exact zeros at ignored pixels
    return gx


@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [2, 3, 4, 5, 21, 40, 256])
def test_loss_and_gradient_match_composition(K, layout):
    _check(_logits(K, layout, K), _labels(K, K), K, f"K={K} {layout}")
    x = _logits(K, layout, K + 1).requires_grad_(True)   # the Dice term alone (ce_weight = 0)
    y = _labels(K, K + 1)
    loss = dice_loss(x, y)
    (gx,) = torch.autograd.grad(loss, x)
    xr = x.detach().double().requires_grad_(True)
    lr = composed(xr, y, K, ce_weight=0.0)
    (gr,) = torch.autograd.grad(lr, xr)
    dl, dg = abs(loss.item() - lr.item()), _rel_l2(gx, gr)
    print(f"K={K} {layout} dice alone: loss |d| {dl:.3e}, grad rel L2 {dg:.3e}")
    assert dl < 1e-4 and dg < 1e-4
    assert (gx[0, :, :3] == 0).all() and (gx[-1, :, 5, 7] == 0).all()


@pytest.mark.parametrize("include_background", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [3, 21])
def test_class_weights_and_background(K, layout, weighted, include_background):
    w = (torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(200 + K)) + 0.5) \
        if weighted else None
    _check(_logits(K, layout, 30 + K), _labels(K, 30 + K), K, f"K={K} {layout} w={weighted} bg={include_background}",
           weight=w, ce_weight=0.7, dice_weight=1.3, smooth=0.5, include_background=include_background)


@pytest.mark.parametrize("K", [3, 21])
def test_three_samples_do_not_mix(K):
    """N = 3: a block's sums and table are one sample's.  With the Dice term alone a sample's gradient depends
    on that sample only: changing the other two leaves it bit-identical."""
    shape = (3, H, W)
    x, y = _logits(K, "nhwc_view", 40 + K, shape), _labels(K, 40 + K, shape)
    _check(x.detach().clone().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), y, K, f"K={K} N=3")
    xa = x.detach().clone().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    xb = xa.detach().clone().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    xb[0] += 1.5
    xb[2] = -xb[2]
    xb.requires_grad_(True)
    (ga,) = torch.autograd.grad(dice_loss(xa, y), xa)
    (gb,) = torch.autograd.grad(dice_loss(xb, y), xb)
    assert torch.equal(ga[1], gb[1]) and not torch.equal(ga[0], gb[0]) and not torch.equal(ga[2], gb[2])


@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [3, 21])
def test_several_blocks_per_sample(K, layout):
    """1 x K x 70 x 70: 4,900 pixels, 20 blocks of one sample: the second reduction stage is live."""
    shape = (1, 70, 70)
    _check(_logits(K, layout, 50 + K, shape), _labels(K, 50 + K, shape), K, f"K={K} {layout} 70x70")


@pytest.mark.parametrize("K", [4, 5])
def test_misaligned_buffer(K):
    """A buffer that starts 4 bytes past a 16-byte boundary: no vector access, no LDS tiles."""
    g = torch.Generator(device=DEV).manual_seed(K)
    flat = torch.randn(N * H * W * K + 1, device=DEV, generator=g)
    x = flat[1:].view(N, H, W, K).permute(0, 3, 1, 2)
    assert x.data_ptr() % 16 == 4
    _check(x, _labels(K, 60 + K), K, f"K={K} misaligned")


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("shape", [(2, 17, 23), (1, 70, 70)])
def test_binary(shape, soft):
    g = torch.Generator(device=DEV).manual_seed(shape[1])
    x = (torch.randn(shape, device=DEV, generator=g) * 2).requires_grad_(True)
    t = torch.rand(shape, device=DEV, generator=g)
    if not soft:
        t = (t > 0.6).float()
    for bw, dw in ((1.0, 1.0), (0.0, 1.0), (0.8, 1.2)):
        loss = bce_dice_loss(x, t, bw, dw, 1.0) if bw else dice_loss(x, t)
        (gx,) = torch.autograd.grad(loss, x)
        xr = x.detach().double().requires_grad_(True)
        lr = composed_binary(xr, t.double(), bw, dw, 1.0)
        (gr,) = torch.autograd.grad(lr, xr)
        dl, dg = abs(loss.item() - lr.item()), _rel_l2(gx, gr)
        print(f"binary {shape} soft={soft} bce_weight={bw}: loss |d| {dl:.3e}, grad rel L2 {dg:.3e}")
        assert dl < 1e-4 and dg < 1e-4
        assert gx.shape == x.shape and gx.dtype == torch.float32
    x4 = x.detach().unsqueeze(1).requires_grad_(True)   # [N, 1, H, W] logits
    l4 = bce_dice_loss(x4, t)
    (g4,) = torch.autograd.grad(l4, x4)
    l3 = bce_dice_loss(x, t)
    (g3,) = torch.autograd.grad(l3, x)
    assert torch.equal(l4, l3) and torch.equal(g4.squeeze(1), g3)


@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [3, 21])
def test_all_pixels_ignored(layout, K):
    x = _logits(K, layout, 1).requires_grad_(True)
    y = torch.full((N, H, W), -100, device=DEV, dtype=torch.int64)
    ld = dice_loss(x, y)
    (gd,) = torch.autograd.grad(ld, x)
    lc = ce_dice_loss(x, y)
    (gc,) = torch.autograd.grad(lc, x)
    torch.cuda.synchronize()
    assert ld.item() == 0.0 and (gd == 0).all()      # every dice is smooth / smooth = 1 exactly
    assert torch.isnan(lc) and (gc == 0).all()       # the cross-entropy's rule


def test_one_sample_all_ignored():
    K = 3
    x, y = _logits(K, "nhwc_view", 70), _labels(K, 70)
    y[0] = -100
    y[1, :3] = -100
    x = x.requires_grad_(True)
    loss = ce_dice_loss(x, y)
    (gx,) = torch.autograd.grad(loss, x)
    xr = x.detach().double().requires_grad_(True)
    lr = composed(xr, y, K)
    (gr,) = torch.autograd.grad(lr, xr)
    assert abs(loss.item() - lr.item()) < 1e-4 and _rel_l2(gx, gr) < 1e-4
    assert (gx[0] == 0).all() and (gx[1, :, :3] == 0).all()


@pytest.mark.parametrize("K", [4, 21, 0])
def test_deterministic(K):
    """Two runs bit-identical; K = 0 stands for the binary form."""
    outs = []
    if K:
        x, y = _logits(K, "nhwc_view", 7), _labels(K, 7)
        w = torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(300 + K)) + 0.5
    else:
        g = torch.Generator(device=DEV).manual_seed(8)
        x, y = torch.randn(1, 70, 70, device=DEV, generator=g), torch.rand(1, 70, 70, device=DEV, generator=g)
    for _ in range(2):
        if K:
            xi = x.clone().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
            loss = ce_dice_loss(xi, y, weight=w)
        else:
            xi = x.clone().requires_grad_(True)
            loss = bce_dice_loss(xi, y)
        (g,) = torch.autograd.grad(loss, xi)
        outs.append((loss.detach().clone(), g.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_zero_dice_weight_is_the_existing_loss_bit_for_bit():
    K = 3
    x, y = _logits(K, "nhwc_view", 9).requires_grad_(True), _labels(K, 9)
    l1, l2 = ce_dice_loss(x, y, dice_weight=0.0), cross_entropy(x, y)
    (g1,), (g2,) = torch.autograd.grad(l1, x), torch.autograd.grad(l2, x)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    xb = torch.randn(N, H, W, device=DEV, requires_grad=True)
    t = (torch.rand(N, H, W, device=DEV) > 0.5).float()
    l1, l2 = bce_dice_loss(xb, t, dice_weight=0.0), bce_with_logits(xb, t)
    (g1,), (g2,) = torch.autograd.grad(l1, xb), torch.autograd.grad(l2, xb)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


# ------------------------------------------------------------------------------------------------
def test_unet_ce_dice_step_runs_three_loss_kernels():
    """engine UNet(out_classes=3) + ce+dice: from the head's forward to the head's data gradient only dlmpi::
    kernels run, among them exactly one fused forward, one finish, one fused backward and one pad-cast --
    the passes of the cross-entropy alone."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    from deeplearning_mpi_amd.models import UNet

    torch.manual_seed(0)
    m = UNet(out_classes=3).to(DEV)
    x = torch.randn(2, 3, 32, 32, device=DEV)
    y = torch.randint(3, (2, 32, 32), device=DEV)
    backward(ce_dice_loss(m(x), y))           # warm-up: arena, cached unit seed gradient
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        backward(ce_dice_loss(m(x), y))
        torch.cuda.synchronize()
    kernels = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
    names = [e.name for e in kernels]
    if not names:
        pytest.fail("the profiler recorded no device kernels")
    first = next(i for i, n in enumerate(names) if "head1x1_kernel" in n)
    last = next(i for i, n in enumerate(names) if "head_dgrad_bn_kernel" in n)
    assert first < last
    between = names[first:last + 1]
    foreign = [n for n in between if "dlmpi::" not in n]
    assert not foreign, foreign
    for part in ("ce_dice_fwd_kernel", "ce_dice_finish_kernel", "ce_dice_bwd_kernel", "nhwc_pad_cast_kernel"):
        assert sum(part in n for n in between) == 1, (part, between)
    assert not any("pixel_ce_" in n for n in between), between


def _run_steps(model, batches, graph):
    from deeplearning_mpi_amd.optim import Adam, clip_grad_norm_
    from deeplearning_mpi_amd.utils.graphs import CapturedStep

    opt = Adam(model.parameters(), lr=1e-3)
    x, y = batches[0][0].clone(), batches[0][1].clone()

    def step():
        opt.zero_grad()
        loss = ce_dice_loss(model(x), y)
        loss.backward()
        clip_grad_norm_(model.parameters(), 1.0, optimizer=opt)
        opt.step()
        return loss

    cs = CapturedStep(step, warmup=1, inputs=(x, y), enabled=graph)
    losses = []
    for bx, by in batches:
        cs.set_inputs(bx, by)
        losses.append(cs().clone())
    torch.cuda.synchronize()
    if graph:
        assert cs.graph is not None
    return torch.stack(losses), [p.detach().clone() for p in model.parameters()], \
        [b.detach().clone() for b in model.buffers()]


def test_unet_ce_dice_graph_replay_matches_eager():
    """One warm-up step, the capture, two replays: bit-identical to the same four eager steps."""
    from deeplearning_mpi_amd.models import UNet

    g = torch.Generator(device=DEV).manual_seed(4)
    batches = [(torch.randn(2, 3, 64, 64, device=DEV, generator=g),
                torch.randint(3, (2, 64, 64), device=DEV, generator=g)) for _ in range(4)]
    torch.manual_seed(0)
    m1 = UNet(out_classes=3).to(DEV)
    m2 = copy.deepcopy(m1)
    l1, p1, b1 = _run_steps(m1, batches, graph=False)
    l2, p2, b2 = _run_steps(m2, batches, graph=True)
    assert torch.equal(l1, l2), (l1, l2)
    for a, b in zip(p1, p2):
        assert torch.equal(a, b)
    for a, b in zip(b1, b2):
        assert torch.equal(a, b)


def test_unet_ce_dice_training_decreases_loss():
    from deeplearning_mpi_amd.models import UNet
    from deeplearning_mpi_amd.optim import Adam, clip_grad_norm_

    torch.manual_seed(0)
    m = UNet(out_classes=3, in_channels=1).to(DEV)
    opt = Adam(m.parameters(), lr=1e-3)
    x = torch.randn(2, 1, 32, 32, device=DEV)
    t = (x[:, 0] > 0).long() + (x[:, 0] > 1).long()
    losses = []
    for _ in range(30):
        loss = ce_dice_loss(m(x), t)
        opt.zero_grad()
        loss.backward()
        clip_grad_norm_(m.parameters(), 1.0, optimizer=opt)
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


def test_trainer_loss_ce_dice(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "pytorch/unet/train.py", "--synthetic", "--image_size", "32", "--num_classes",
                        "3", "--loss", "ce+dice", "--num_epochs", "1", "--batch_size", "4", "--eval_every", "1",
                        "--workers", "0", "--log_dir", str(tmp_path / "logs"), "--model_dir", str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    (log,) = glob.glob(str(tmp_path / "logs" / "training_log_*.log"))
    text = open(log).read()
    line = [ln for ln in text.splitlines() if "| Loss:" in ln][0]
    loss = float(line.split("Loss:")[1].split("|")[0])
    assert loss == loss and 0.0 < loss < 1e3, line
    assert [ln for ln in text.splitlines() if "Dice Score:" in ln], text
