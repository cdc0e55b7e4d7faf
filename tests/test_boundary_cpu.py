"""The boundary loss without a GPU: RefBackend's distance transform on the cases of the GPU test (exact), its signed
map, the public functions on fp64 CPU tensors against tests/boundary_ref.py (loss 1e-12, gradient 1e-10), the limits,
the argument refusals and the trainer's flags."""
import pytest
import torch

import boundary_ref as R
from deeplearning_mpi_amd.apps import segmentation as seg
from deeplearning_mpi_amd.ops import (BCEBoundaryLoss, BCEWithLogitsLoss, BoundaryLoss, CEBoundaryLoss, CrossEntropyLoss,
                                      RefBackend, bce_boundary_loss, bce_with_logits, boundary_loss, ce_boundary_loss,
                                      cross_entropy, edt_squared, signed_distance_map)

SHAPES = R.edt_shapes(RefBackend.edt_strip, RefBackend.edt_strip_rows)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", R.PATTERNS)
def test_edt_exact(name, shape):
    mask, want = R.edt_case(name, *shape)
    assert torch.equal(edt_squared(mask), want)


@pytest.mark.parametrize("K", [3, "binary"])
def test_signed_map(K):
    if K == "binary":
        _, t, ref = R.sigmoid_inputs(2)
        R.check_signed_map(signed_distance_map(t), ref)
    else:
        _, y, ref = R.softmax_inputs(K, 1)
        R.check_signed_map(signed_distance_map(y, K), ref)
        assert (ref[:, K - 1] == 0).all() and (ref[0, :, :3] >= 0).all()   # an absent class; ignored rows are outside


def _close(loss, x, ref):
    gx = torch.autograd.grad(loss, x)[0]
    assert abs(loss.item() - ref[0].item()) < 1e-12 and R.rel_l2(gx, ref[1]) < 1e-10
    return gx


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.5)], ids=str)
@pytest.mark.parametrize("background", [True, False])
@pytest.mark.parametrize("K", [2, 5])
def test_softmax_matches_reference(K, background, weights):
    xc, y, phi = R.softmax_inputs(K, 1)
    x = xc.permute(0, 3, 1, 2).double().requires_grad_(True)
    loss = ce_boundary_loss(x, y, include_background=background, ce_weight=weights[0], boundary_weight=weights[1])
    gx = _close(loss, x, R.softmax_reference(x, y, phi, background, *weights))
    assert (gx.permute(0, 2, 3, 1)[(y < 0) | (y >= K)] == 0).all()


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.5)], ids=str)
def test_sigmoid_matches_reference(weights):
    xc, t, phi = R.sigmoid_inputs(2)
    x = xc.unsqueeze(1).double().requires_grad_(True)
    _close(bce_boundary_loss(x, t, bce_weight=weights[0], boundary_weight=weights[1]), x,
           R.sigmoid_reference(xc, t, phi, *weights))


def test_limits_and_refusals():
    xc, y, _ = R.softmax_inputs(3, 1)
    x = xc.permute(0, 3, 1, 2).requires_grad_(True)
    loss = boundary_loss(x, torch.full_like(y, -100))            # nothing valid
    assert loss.item() == 0 and (torch.autograd.grad(loss, x)[0] == 0).all()
    assert torch.equal(ce_boundary_loss(x, y, boundary_weight=0.0), cross_entropy(x, y))
    t = (y == 1).float()
    assert torch.equal(bce_boundary_loss(x[:, 0], t, boundary_weight=0.0), bce_with_logits(x[:, 0], t))
    a = ce_boundary_loss(x, y, dist=signed_distance_map(y, 3), boundary_weight=torch.tensor([0.5]))
    assert torch.equal(a, ce_boundary_loss(x, y, boundary_weight=0.5))
    for bad in (dict(boundary_weight=-1.0), dict(ce_weight=0.0, boundary_weight=0.0), dict(ce_weight=float("nan")),
                dict(boundary_weight=torch.ones(2)), dict(dist=torch.zeros(1, 3, 2, 2))):
        with pytest.raises(ValueError):
            ce_boundary_loss(x, y, **bad)
    with pytest.raises(ValueError):
        bce_boundary_loss(x[:, 0], y)                             # an integer target


def test_app_flags_and_ramp():
    assert type(seg.build_criterion(seg.parse_args([]))) is BCEWithLogitsLoss   # the defaults build today's criteria
    assert type(seg.build_criterion(seg.parse_args(["--num_classes", "3"]))) is CrossEntropyLoss
    for k in ("1", "3"):
        assert type(seg.build_criterion(seg.parse_args(["--num_classes", k, "--loss", "boundary"]))) is BoundaryLoss
    crit = seg.build_criterion(seg.parse_args(["--loss", "ce+boundary"]))
    assert type(crit) is BCEBoundaryLoss and (crit.bce_weight, crit.boundary_weight) == (1.0, 0.01)
    args = seg.parse_args(["--num_classes", "3", "--loss", "ce+boundary", "--ignore_index", "255", "--boundary_weight",
                           "0.25", "--boundary_ramp", "0.125", "--boundary_background", "0"])
    crit = seg.build_criterion(args)
    assert type(crit) is CEBoundaryLoss
    assert (crit.ignore_index, crit.include_background, crit.ce_weight, crit.boundary_weight) == (255, False, 1.0, 0.25)
    for epoch in (0, 3):                                          # the ramp: A + D * epoch in one device scalar
        seg.set_boundary_epoch(crit, args, epoch, torch.device("cpu"))
        assert crit.boundary_weight.dtype == torch.float32 and crit.boundary_weight.item() == 0.25 + 0.125 * epoch
    plain = seg.build_criterion(seg.parse_args([]))
    seg.set_boundary_epoch(plain, args, 1, torch.device("cpu"))   # other criteria are left alone
    assert not hasattr(plain, "boundary_weight")
    for argv in (["--loss", "boundary", "--ohem_ratio", "0.25"], ["--loss", "ce+boundary", "--ohem_ratio", "0.25"],
                 ["--loss", "ce+boundary", "--boundary_weight", "-1"], ["--loss", "ce+boundary", "--boundary_ramp", "-1"]):
        with pytest.raises(SystemExit):
            seg.parse_args(argv)
