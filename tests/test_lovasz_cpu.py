"""The Lovasz losses without a GPU: the closed-form Jaccard gradient against the paper's cumulative form, RefBackend's
sort on the cases of the GPU test, the public functions on fp64 CPU tensors against tests/lovasz_ref.py (loss 1e-12,
gradient 1e-10), the argument refusals and the trainer's flags."""
import pytest
import torch

import lovasz_ref as R
from deeplearning_mpi_amd.apps import segmentation as seg
from deeplearning_mpi_amd.ops import (BCELovaszLoss, BCEWithLogitsLoss, CELovaszLoss, CrossEntropyLoss, LovaszHingeLoss,
                                      LovaszSoftmaxLoss, RefBackend, bce_lovasz_loss, ce_lovasz_loss, lovasz_hinge,
                                      lovasz_softmax)

TILE = RefBackend.lovasz_tile


def test_closed_form_is_the_papers_gradient():
    g = torch.Generator().manual_seed(3)
    for n, share in ((1, 0.5), (1, 1.1), (37, 0.0), (37, 1.1), (1000, 0.3)):   # incl. no fg at all, fg only
        fg = torch.rand(n, generator=g) < share
        assert (R.closed_form(fg) - R.lovasz_grad(fg.double())).abs().max() < 1e-12


@pytest.mark.parametrize("L", [1, 255, TILE - 1, TILE, TILE + 1, 70001])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", R.PATTERNS)
def test_sort_and_jaccard_gradient(name, S, L):
    R.check_sort(RefBackend("cpu", torch.float32), "cpu", name, S, L)


def _close(loss, x, ref):
    gx = torch.autograd.grad(loss, x)[0]
    assert abs(loss.item() - ref[0].item()) < 1e-12 and R.rel_l2(gx, ref[1]) < 1e-10
    return gx


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.5)], ids=str)
@pytest.mark.parametrize("classes", ["present", "all"])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("K", [2, 5])
def test_softmax_matches_reference(K, per_image, classes, weights):
    xc, y = R.softmax_inputs(K, 1, absent=True)
    x = xc.permute(0, 3, 1, 2).double().requires_grad_(True)
    loss = ce_lovasz_loss(x, y, classes=classes, per_image=per_image, ce_weight=weights[0], lovasz_weight=weights[1])
    gx = _close(loss, x, R.softmax_reference(x, y, classes, per_image, *weights))
    assert (gx.permute(0, 2, 3, 1)[(y < 0) | (y >= K)] == 0).all()


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.5)], ids=str)
@pytest.mark.parametrize("per_image", [False, True])
def test_hinge_matches_reference(per_image, weights):
    xc, t = R.hinge_inputs(2)
    x = xc.unsqueeze(1).double().requires_grad_(True)
    loss = bce_lovasz_loss(x, t, per_image=per_image, bce_weight=weights[0], lovasz_weight=weights[1])
    _close(loss, x, R.hinge_reference(xc, t, per_image, *weights))


def test_limits_and_refusals():
    xc, y = R.softmax_inputs(3, 1)
    x = xc.permute(0, 3, 1, 2).requires_grad_(True)
    loss = lovasz_softmax(x, torch.full_like(y, -100))          # nothing to count
    assert loss.item() == 0 and (torch.autograd.grad(loss, x)[0] == 0).all()
    assert lovasz_hinge(xc[..., 0], (y > 0).float()).item() > 0
    for bad in (dict(classes="some"), dict(lovasz_weight=-1.0), dict(ce_weight=0.0, lovasz_weight=0.0),
                dict(ce_weight=float("nan"))):
        with pytest.raises(ValueError):
            ce_lovasz_loss(x, y, **bad)
    with pytest.raises(ValueError):
        bce_lovasz_loss(xc[..., 0], y, bce_weight=1.0)            # an integer target


def test_app_flags():
    assert type(seg.build_criterion(seg.parse_args([]))) is BCEWithLogitsLoss   # the defaults build today's criteria
    assert type(seg.build_criterion(seg.parse_args(["--num_classes", "3"]))) is CrossEntropyLoss
    crit = seg.build_criterion(seg.parse_args(["--loss", "lovasz"]))
    assert type(crit) is LovaszHingeLoss and crit.per_image is True
    crit = seg.build_criterion(seg.parse_args(["--loss", "ce+lovasz", "--lovasz_weight", "0.5", "--lovasz_per_image", "0"]))
    assert type(crit) is BCELovaszLoss and (crit.per_image, crit.bce_weight, crit.lovasz_weight) == (False, 1.0, 0.5)
    crit = seg.build_criterion(seg.parse_args(["--num_classes", "3", "--loss", "lovasz", "--ignore_index", "255",
                                               "--lovasz_classes", "all"]))
    assert type(crit) is LovaszSoftmaxLoss and (crit.per_image, crit.classes, crit.ignore_index) == (False, "all", 255)
    crit = seg.build_criterion(seg.parse_args(["--num_classes", "3", "--loss", "ce+lovasz", "--lovasz_per_image", "1"]))
    assert type(crit) is CELovaszLoss and (crit.per_image, crit.ce_weight, crit.lovasz_weight) == (True, 1.0, 1.0)
    for argv in (["--loss", "lovasz", "--ohem_ratio", "0.25"], ["--loss", "ce+lovasz", "--ohem_ratio", "0.25"],
                 ["--loss", "ce+lovasz", "--lovasz_weight", "-1"], ["--loss", "lovasz", "--lovasz_classes", "few"]):
        with pytest.raises(SystemExit):
            seg.parse_args(argv)
