"""The Lovasz-Softmax / Lovasz hinge kernels (csrc/kernels/lovasz.hip) against the plain fp64 reference of
tests/lovasz_ref.py: the segmented radix sort and the Jaccard gradient exactly, the loss and the gradient end to end,
ties and limits, and determinism under graph replay (tests/lovasz_graph_replay.py).

Tolerances: the permutation is exact; g is an fp64 value rounded once to fp32 (6e-8), checked at 1e-6 relative; the
loss is continuous in the errors and takes the plain pixel loss's |d| < 1e-4 (tests/test_pixel_ce_gpu.py); the
gradient (relative L2 < 1e-4) is compared where the reference has asserted that both precisions rank alike."""
import os
import subprocess
import sys

import pytest
import torch

import lovasz_ref as R
from deeplearning_mpi_amd.ops import (bce_lovasz_loss, bce_with_logits, ce_lovasz_loss, cross_entropy, lovasz_softmax,
                                      make_backend)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 2048   # asserted below to be the backend's


def _layout(x, layout):   # class-last CPU storage -> device [N, K, H, W]
    x = x.to(DEV).permute(0, 3, 1, 2)
    return x if layout == "nhwc_view" else x.contiguous()


@pytest.mark.parametrize("L", [1, 255, TILE - 1, TILE, TILE + 1, 70001])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", R.PATTERNS)
def test_sort_and_jaccard_gradient(name, S, L):
    be = make_backend(DEV)
    assert be.lovasz_tile == TILE
    R.check_sort(be, DEV, name, S, L)


@pytest.mark.parametrize("classes", ["present", "all"])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [2, 3, 4, 5, 21, 40])
def test_softmax_loss_matches_fp64(K, layout, per_image, classes):
    xc, y = R.softmax_inputs(K, 1, absent=True)
    x = _layout(xc, layout)
    for w in ((0.0, 1.0), (1.0, 0.5)):
        loss = ce_lovasz_loss(x, y.to(DEV), classes=classes, per_image=per_image, ce_weight=w[0], lovasz_weight=w[1])
        d = abs(loss.item() - R.softmax_reference(x.cpu(), y, classes, per_image, *w)[0].item())
        print(f"K={K} {layout} per_image={per_image} {classes} {w}: loss |d| {d:.3e}")
        assert d < 1e-4


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("channel", [False, True])
def test_hinge_loss_matches_fp64(channel, per_image):
    xc, t = R.hinge_inputs(2)
    x = (xc.unsqueeze(1) if channel else xc).to(DEV)
    for w in ((0.0, 1.0), (1.0, 0.5)):
        loss = bce_lovasz_loss(x, t.to(DEV), per_image=per_image, bce_weight=w[0], lovasz_weight=w[1])
        d = abs(loss.item() - R.hinge_reference(xc, t, per_image, *w)[0].item())
        print(f"hinge channel={channel} per_image={per_image} {w}: loss |d| {d:.3e}")
        assert d < 1e-4


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.5)], ids=str)
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [2, 3, 5, 21])
def test_softmax_gradient_matches_fp64(K, layout, per_image, weights):
    xc, y = R.softmax_inputs(K, R.GRAD_SEEDS[K], R.GRAD_SHAPES[K])
    x = _layout(xc, layout).requires_grad_(True)
    loss = ce_lovasz_loss(x, y.to(DEV), per_image=per_image, ce_weight=weights[0], lovasz_weight=weights[1])
    (gx,) = torch.autograd.grad(loss, x)
    lr, gr = R.softmax_reference(x.cpu(), y, "present", per_image, *weights, min_gap=1e-5)
    dl, dg = abs(loss.item() - lr.item()), R.rel_l2(gx, gr)
    print(f"K={K} {layout} per_image={per_image} {weights}: loss |d| {dl:.3e}, grad rel L2 {dg:.3e}")
    assert dl < 1e-4 and dg < 1e-4
    assert gx.stride() == x.stride() and gx.dtype == torch.float32
    assert (gx.permute(0, 2, 3, 1)[((y < 0) | (y >= K)).to(DEV)] == 0).all()   # exact zeros at invalid pixels


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.5)], ids=str)
@pytest.mark.parametrize("per_image", [False, True])
def test_hinge_gradient_matches_fp64(per_image, weights):
    xc, t = R.hinge_inputs(R.GRAD_SEEDS["hinge"], R.GRAD_SHAPES["hinge"])
    x = xc.unsqueeze(1).to(DEV).requires_grad_(True)
    loss = bce_lovasz_loss(x, t.to(DEV), per_image=per_image, bce_weight=weights[0], lovasz_weight=weights[1])
    (gx,) = torch.autograd.grad(loss, x)
    lr, gr = R.hinge_reference(xc, t, per_image, *weights, min_gap=1e-5)
    dl, dg = abs(loss.item() - lr.item()), R.rel_l2(gx, gr)
    print(f"hinge per_image={per_image} {weights}: loss |d| {dl:.3e}, grad rel L2 {dg:.3e}")
    assert dl < 1e-4 and dg < 1e-4 and gx.stride() == x.stride()


def test_ties_and_limits():
    xc, y = R.softmax_inputs(3, 11, (1, R.H, R.W))
    x = _layout(torch.cat([xc, xc]), "nhwc_view").requires_grad_(True)
    y2 = torch.cat([y, y]).to(DEV)
    (gx,) = torch.autograd.grad(lovasz_softmax(x, y2, per_image=True), x)
    assert torch.equal(gx[0], gx[1]) and gx.abs().sum() > 0          # one sample twice: equal gradients
    for f, plain, t in ((ce_lovasz_loss, cross_entropy, y2), (bce_lovasz_loss, bce_with_logits, (y2 == 1).float())):
        xs = x if f is ce_lovasz_loss else x[:, :1]
        a, b = f(xs, t, lovasz_weight=0.0), plain(xs, t)             # the plain kernels, bit for bit
        assert torch.equal(a, b) and torch.equal(torch.autograd.grad(a, x)[0], torch.autograd.grad(b, x)[0])
    loss = lovasz_softmax(x, torch.full_like(y2, -100))              # an all-ignored batch
    assert loss.item() == 0 and (torch.autograd.grad(loss, x)[0] == 0).all()


def test_deterministic_and_follows_inputs_under_replay():
    """tests/lovasz_graph_replay.py in a process of its own (as tests/test_ohem_gpu.py's replay test)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "lovasz_graph_replay.py")], cwd=root,
                       env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "replays equal eager: 4" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
