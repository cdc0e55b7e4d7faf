"""Pixel-wise softmax cross-entropy and segmentation counts (csrc/kernels/pixel_ce.hip) against torch:
both native layouts, class weights, ignored and out-of-range labels, the all-ignored batch,
run-to-run determinism, the argmax counts with the Dice / IoU built on them, and a K-class UNet step
that launches no ATen kernel between the head's forward and its data gradient.

Tolerances (__expf / __logf arithmetic, as tests/test_kernels_gpu.py::test_losses_eval_optim): loss
|d| < 1e-4, gradient relative L2 < 1e-4 against F.cross_entropy on the fp64 copy of the fp32 logits."""
import pytest
import torch
import torch.nn.functional as F

from deeplearning_mpi_amd.ops import backward, cross_entropy, dice_multiclass, mean_iou, seg_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, H, W = 2, 17, 23   # 391 pixels per sample: no multiple of 64 or 256, tail lanes and partial blocks live


def _logits(K, layout, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.randn(N, H, W, K, device=DEV, generator=g)
    x = base.permute(0, 3, 1, 2)
    return x if layout == "nhwc_view" else x.contiguous()


def _labels(K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed + 100)
    y = torch.randint(K, (N, H, W), device=DEV, generator=g)
    y[0, :3] = -100
    y[1, 5, 7] = K + 3   # out of range: ignored as well
    return y


def _rel_l2(a, ref):
    a, ref = a.double().flatten(), ref.double().flatten()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [2, 3, 5, 21])
def test_loss_and_gradient_match_torch(K, layout, weighted):
    x = _logits(K, layout, K).requires_grad_(True)
    y = _labels(K, K)
    w = (torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(200 + K)) + 0.5) \
        if weighted else None
    loss = cross_entropy(x, y, weight=w, ignore_index=-100)
    (gx,) = torch.autograd.grad(loss, x)
    xr = x.detach().double().requires_grad_(True)
    yr = torch.where((y >= 0) & (y < K), y, torch.full_like(y, -100))
    lr = F.cross_entropy(xr, yr, weight=w.double() if weighted else None, ignore_index=-100)
    (gr,) = torch.autograd.grad(lr, xr)
    torch.cuda.synchronize()
    dl, dg = abs(loss.item() - lr.item()), _rel_l2(gx, gr)
    print(f"K={K} {layout} weighted={weighted}: loss |d| {dl:.3e}, grad rel L2 {dg:.3e}")
    assert dl < 1e-4
    assert dg < 1e-4
    assert gx.stride() == x.stride() and gx.dtype == torch.float32
    assert (gx[0, :, :3] == 0).all() and (gx[1, :, 5, 7] == 0).all()   # exact zeros at ignored pixels


@pytest.mark.parametrize("K,misaligned", [(32, False), (40, False), (256, False), (5, True), (4, True)])
def test_loss_and_gradient_other_kernel_paths(K, misaligned):
    """Class-last logits beyond the issue's K: 32 (the widest 256-pixel LDS tile), 40 and 256 (narrower
    tiles), and a buffer that starts 4 bytes past a 16-byte boundary (no vector access, no LDS tiles)."""
    g = torch.Generator(device=DEV).manual_seed(K)
    flat = torch.randn(N * H * W * K + 1, device=DEV, generator=g)
    x = flat[1:] if misaligned else flat[:-1]
    x = x.view(N, H, W, K).permute(0, 3, 1, 2).requires_grad_(True)
    assert (x.data_ptr() % 16 != 0) == misaligned
    y = _labels(K, K)
    loss = cross_entropy(x, y)
    (gx,) = torch.autograd.grad(loss, x)
    xr = x.detach().double().requires_grad_(True)
    yr = torch.where((y >= 0) & (y < K), y, torch.full_like(y, -100))
    lr = F.cross_entropy(xr, yr)
    (gr,) = torch.autograd.grad(lr, xr)
    torch.cuda.synchronize()
    assert abs(loss.item() - lr.item()) < 1e-4
    assert _rel_l2(gx, gr) < 1e-4
    assert gx.stride() == x.stride()
    assert (gx[0, :, :3] == 0).all() and (gx[1, :, 5, 7] == 0).all()


@pytest.mark.parametrize("K", [3, 21])
@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
def test_all_pixels_ignored(layout, K):
    x = _logits(K, layout, 1).requires_grad_(True)
    y = torch.full((N, H, W), -100, device=DEV, dtype=torch.int64)
    loss = cross_entropy(x, y)
    (gx,) = torch.autograd.grad(loss, x)
    torch.cuda.synchronize()
    assert torch.isnan(loss)
    assert (gx == 0).all()


@pytest.mark.parametrize("K", [4, 21])
def test_deterministic(K):
    x = _logits(K, "nhwc_view", 7)
    y = _labels(K, 7)
    w = torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(300 + K)) + 0.5
    outs = []
    for _ in range(2):
        xi = x.clone().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
        loss = cross_entropy(xi, y, weight=w)
        (g,) = torch.autograd.grad(loss, xi)
        outs.append((loss.detach().clone(), g.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _counts_ref(x, y, K):
    pred = x.argmax(1)
    keep = (y >= 0) & (y < K)
    out = torch.zeros(x.shape[0], K, 3, dtype=torch.int64, device=x.device)
    for n in range(x.shape[0]):
        p, t = pred[n][keep[n]], y[n][keep[n]]
        out[n, :, 0] = torch.bincount(p[p == t], minlength=K)
        out[n, :, 1] = torch.bincount(p, minlength=K)
        out[n, :, 2] = torch.bincount(t, minlength=K)
    return out


def _dice_ref(c):
    c = c[:, 1:].double()
    uni = c[..., 1] + c[..., 2]
    return torch.where(uni > 0, (2 * c[..., 0] + 1e-8) / (uni + 1e-8), torch.ones_like(uni)).mean(1)


def _miou_ref(c):
    c = c.sum(0).double()
    union = c[:, 1] + c[:, 2] - c[:, 0]
    has = union > 0
    return (c[:, 0][has] / union[has]).mean()


@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [2, 5, 21])
def test_seg_counts_exact(K, layout):
    x = _logits(K, layout, 10 + K)
    top2 = x.topk(2, dim=1).values
    assert (top2[:, 0] - top2[:, 1]).min() > 0   # no ties: the argmax is unambiguous
    y = _labels(K, 10 + K)
    c = seg_counts(x, y)
    torch.cuda.synchronize()
    ref = _counts_ref(x, y, K)
    assert c.dtype == torch.int64 and c.shape == (N, K, 3)
    assert torch.equal(c, ref)
    assert int(c[..., 2].sum()) == int(((y >= 0) & (y < K)).sum())
    assert torch.allclose(dice_multiclass(x, y).double(), _dice_ref(ref), atol=1e-6)
    assert abs(mean_iou(x, y).item() - _miou_ref(ref).item()) < 1e-6


def test_argmax_tie_goes_to_the_lowest_index():
    x = torch.zeros(1, 4, 2, 3, device=DEV)
    x[0, 1] = 2.0
    x[0, 3] = 2.0          # classes 1 and 3 tie everywhere: 1 wins
    x[0, :, 0, 0] = 0.0    # four-way tie at one pixel: 0 wins
    y = torch.tensor([[[0, 1, 3], [1, 3, 3]]], device=DEV)
    c = seg_counts(x, y)
    torch.cuda.synchronize()
    assert c[0].tolist() == [[1, 1, 1], [2, 5, 2], [0, 0, 0], [0, 0, 3]]


def test_dice_absent_class_scores_one_and_ignored_pixels_count_nowhere():
    K = 4
    x = _logits(K, "nhwc_view", 3).clone()
    x[1, 3] = -50.0                  # class 3 never predicted in sample 1 ...
    y = _labels(K, 3)
    y[1][y[1] == 3] = 0              # ... nor present there
    c = seg_counts(x, y)
    ref = _counts_ref(x, y, K)
    assert torch.equal(c, ref) and c[1, 3].tolist() == [0, 0, 0]
    d = dice_multiclass(x, y).double()
    want = _dice_ref(ref)
    assert torch.allclose(d, want, atol=1e-6)
    per_class = (2 * ref[1, 1:3, 0].double() + 1e-8) / (ref[1, 1:3, 1] + ref[1, 1:3, 2] + 1e-8).double()
    assert abs(d[1].item() - (per_class.sum().item() + 1.0) / 3) < 1e-6   # the absent class contributes 1.0
    assert int(c[0, :, 2].sum()) == (H - 3) * W                           # 3 ignored rows in sample 0
    assert abs(mean_iou(x, y).item() - _miou_ref(ref).item()) < 1e-6


def test_unet_multiclass_step_launches_no_aten_kernel_on_the_loss_path():
    """engine UNet(out_classes=3) + pixel cross-entropy: from the head's forward to the head's data
    gradient only dlmpi:: kernels run (the logits are read and their gradient written in the engine's NHWC
    layout, the padded gradient comes from the pad-cast), and the pad-cast branch of nchw_to_nhwc is taken."""
    from torch.profiler import ProfilerActivity, profile

    from deeplearning_mpi_amd.models import UNet

    torch.manual_seed(0)
    m = UNet(out_classes=3).to(DEV)
    x = torch.randn(2, 3, 32, 32, device=DEV)
    y = torch.randint(3, (2, 32, 32), device=DEV)
    backward(cross_entropy(m(x), y))           # warm-up: arena, cached unit seed gradient
    torch.cuda.synchronize()
    before = m._be.pad_cast_calls
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        backward(cross_entropy(m(x), y))
        torch.cuda.synchronize()
    assert m._be.pad_cast_calls == before + 1
    from torch.autograd import DeviceType

    kernels = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
    names = [e.name for e in kernels]
    if not names:
        pytest.fail("the profiler recorded no device kernels")
    first = next(i for i, n in enumerate(names) if "head1x1_kernel" in n)
    last = next(i for i, n in enumerate(names) if "head_dgrad_bn_kernel" in n)
    assert first < last
    between = names[first:last + 1]
    assert any("pixel_ce_fwd_kernel" in n for n in between) and any("pixel_ce_bwd_kernel" in n for n in between)
    assert any("nhwc_pad_cast_kernel" in n for n in between)
    foreign = [n for n in between if "dlmpi::" not in n]
    assert not foreign, foreign
