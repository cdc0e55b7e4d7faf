"""The distance transform and the boundary loss kernels (csrc/kernels/edt.hip, boundary.hip) against the plain
references of tests/boundary_ref.py: the transform exactly, the signed map to 1 ulp, loss and gradient against fp64,
the limits, and determinism under graph replay (tests/boundary_graph_replay.py).

Tolerances: the transform is exact integers; the map is an fp64 root rounded once (1 ulp); the loss is a mean of
p * phi, so the pixel losses' |d| < 1e-4 (tests/test_pixel_ce_gpu.py) scales with max(1, max |phi|) of the case; the
gradient takes the Lovasz tests' relative L2 < 1e-4."""
import os
import subprocess
import sys

import pytest
import torch

import boundary_ref as R
from deeplearning_mpi_amd.ops import (bce_boundary_loss, bce_with_logits, boundary_loss, ce_boundary_loss, cross_entropy,
                                      edt_squared, make_backend, signed_distance_map)

pytestmark = pytest.mark.gpu
DEV = "cuda"
STRIP, STRIP_ROWS = 64, 512   # asserted below to be the backend's


def _layout(x, layout):   # class-last CPU storage -> device [N, K, H, W]
    x = x.to(DEV).permute(0, 3, 1, 2)
    return x if layout == "nhwc_view" else x.contiguous()


@pytest.mark.parametrize("shape", R.edt_shapes(STRIP, STRIP_ROWS), ids=str)
@pytest.mark.parametrize("name", R.PATTERNS)
def test_edt_exact(name, shape):
    be = make_backend(DEV)
    assert (be.edt_strip, be.edt_strip_rows) == (STRIP, STRIP_ROWS)
    mask, want = R.edt_case(name, *shape)
    assert torch.equal(edt_squared(mask.to(DEV)).cpu(), want)


@pytest.mark.parametrize("K", [2, 3, 21, "binary"])
def test_signed_map(K):
    if K == "binary":
        _, t, ref = R.sigmoid_inputs(2)
        R.check_signed_map(signed_distance_map(t.to(DEV)), ref)
    else:
        _, y, ref = R.softmax_inputs(K, 1)
        phi = signed_distance_map(y.to(DEV), K)
        R.check_signed_map(phi, ref)
        assert (phi[:, K - 1] == 0).all()                        # an absent class
        full = signed_distance_map(torch.zeros(1, 9, 70, dtype=torch.int64, device=DEV), K)
        assert (full == 0).all()                                 # an image-filling class and K - 1 absent ones


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.5)], ids=str)
@pytest.mark.parametrize("background", [True, False])
@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [2, 3, 5, 21])
def test_softmax_loss_and_gradient_match_fp64(K, layout, background, weights):
    xc, y, phi = R.softmax_inputs(K, 1)
    x = _layout(xc, layout).requires_grad_(True)
    loss = ce_boundary_loss(x, y.to(DEV), include_background=background, ce_weight=weights[0],
                            boundary_weight=weights[1])
    (gx,) = torch.autograd.grad(loss, x)
    lr, gr = R.softmax_reference(x.cpu(), y, phi, background, *weights)
    dl, dg, scale = abs(loss.item() - lr.item()), R.rel_l2(gx, gr), max(1.0, phi.abs().max().item())
    print(f"K={K} {layout} bg={background} {weights}: loss |d| {dl:.3e} (max |phi| {scale:.1f}), grad rel L2 {dg:.3e}")
    assert dl < 1e-4 * scale and dg < 1e-4
    assert gx.stride() == x.stride() and gx.dtype == torch.float32
    assert (gx.permute(0, 2, 3, 1)[((y < 0) | (y >= K)).to(DEV)] == 0).all()   # exact zeros at invalid pixels


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.5)], ids=str)
@pytest.mark.parametrize("channel", [False, True])
def test_sigmoid_loss_and_gradient_match_fp64(channel, weights):
    xc, t, phi = R.sigmoid_inputs(2)
    x = (xc.unsqueeze(1) if channel else xc).to(DEV).requires_grad_(True)
    loss = bce_boundary_loss(x, t.to(DEV), bce_weight=weights[0], boundary_weight=weights[1])
    (gx,) = torch.autograd.grad(loss, x)
    lr, gr = R.sigmoid_reference(xc, t, phi, *weights)
    dl, dg, scale = abs(loss.item() - lr.item()), R.rel_l2(gx, gr), max(1.0, phi.abs().max().item())
    print(f"sigmoid channel={channel} {weights}: loss |d| {dl:.3e} (max |phi| {scale:.1f}), grad rel L2 {dg:.3e}")
    assert dl < 1e-4 * scale and dg < 1e-4 and gx.stride() == x.stride() and gx.dtype == torch.float32


def test_limits():
    xc, y, _ = R.softmax_inputs(3, 11)
    x = _layout(torch.cat([xc[:1], xc[:1]]), "nhwc_view").requires_grad_(True)
    y2 = torch.cat([y[:1], y[:1]]).to(DEV)
    grad = lambda loss: torch.autograd.grad(loss, x)[0]  # noqa: E731
    gx = grad(boundary_loss(x, y2))
    assert torch.equal(gx[0], gx[1]) and gx.abs().sum() > 0          # one sample twice: equal gradients
    for f, plain, t in ((ce_boundary_loss, cross_entropy, y2), (bce_boundary_loss, bce_with_logits, (y2 == 1).float())):
        xs = x if f is ce_boundary_loss else x[:, :1]
        a, b = f(xs, t, boundary_weight=0.0), plain(xs, t)           # a float 0: the plain kernels, bit for bit
        assert torch.equal(a, b) and torch.equal(grad(a), grad(b))
        dist = signed_distance_map(t, 3) if f is ce_boundary_loss else signed_distance_map(t)
        a, b = f(xs, t, boundary_weight=0.5), f(xs, t, boundary_weight=0.5, dist=dist)          # precomputed map
        c = f(xs, t, boundary_weight=torch.full((1,), 0.5, device=DEV))                          # device weight
        assert torch.equal(a, b) and torch.equal(a, c) and not torch.equal(a, plain(xs, t))
        ga = grad(a)
        assert torch.equal(ga, grad(b)) and torch.equal(ga, grad(c))
    loss = boundary_loss(x, torch.full_like(y2, -100))               # an all-ignored batch
    assert loss.item() == 0 and (grad(loss) == 0).all()


def test_deterministic_and_follows_inputs_under_replay():
    """tests/boundary_graph_replay.py in a process of its own (as tests/test_lovasz_gpu.py's replay test)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "boundary_graph_replay.py")], cwd=root,
                       env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "replays equal eager: 4" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
