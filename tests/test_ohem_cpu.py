"""Online hard example mining without a GPU: the public functions on CPU tensors (RefBackend: kthvalue and the >=
rule) against the fp64 reference of tests/ohem_ref.py, the argument refusals, and the app's flags."""
import pytest
import torch

import ohem_ref as R
from deeplearning_mpi_amd.apps import segmentation as seg
from deeplearning_mpi_amd.ops import (BCEWithLogitsLoss, CrossEntropyLoss, OHEMBCEWithLogitsLoss, OHEMCrossEntropyLoss,
                                      ohem_bce_with_logits, ohem_cross_entropy)


@pytest.mark.parametrize("setting", R.SETTINGS, ids=str)
@pytest.mark.parametrize("K,weighted", [(2, False), (21, True)])
def test_softmax_matches_fp64(K, weighted, setting):
    xc, y, w = R.softmax_inputs(K, R.SEEDS[K])
    x = xc.permute(0, 3, 1, 2).requires_grad_(True)
    w = w if weighted else None
    crit = OHEMCrossEntropyLoss(weight=w, keep_ratio=setting[0], min_kept=setting[1], thresh=setting[2])
    loss = crit(x, y)
    lr, gr, sel, k = R.softmax_reference(x, y, w, *setting)
    gx = torch.autograd.grad(loss, x)[0]
    assert abs(loss.item() - lr.item()) < 1e-4 and R.rel_l2(gx, gr) < 1e-4
    assert crit.last_stats["k"].item() == k and crit.last_stats["n_selected"].item() == sel.sum().item()
    assert (gx.permute(0, 2, 3, 1)[~sel] == 0).all()


@pytest.mark.parametrize("setting", R.SETTINGS, ids=str)
def test_binary_matches_fp64(setting):
    xc, t = R.binary_inputs("soft", R.SEEDS["soft"])
    x = xc.unsqueeze(1).requires_grad_(True)
    loss = ohem_bce_with_logits(x, t, *setting)
    lr, gr, sel, _ = R.binary_reference(xc, t, *setting)
    gx = torch.autograd.grad(loss, x)[0]
    assert abs(loss.item() - lr.item()) < 1e-4 and R.rel_l2(gx, gr) < 1e-4 and (gx[:, 0][~sel] == 0).all()


@pytest.mark.parametrize("bad", [dict(keep_ratio=0.0), dict(keep_ratio=1.5), dict(min_kept=0), dict(thresh=0.0),
                                 dict(thresh=1.0)], ids=str)
def test_refusals(bad):
    xc, y, _ = R.softmax_inputs(3, 1)
    with pytest.raises(ValueError):
        ohem_cross_entropy(xc.permute(0, 3, 1, 2), y, **bad)
    with pytest.raises(ValueError):
        ohem_bce_with_logits(xc[..., 0], y.float().clamp(0, 1), **bad)


def test_app_flags():
    args = seg.parse_args([])
    assert (args.ohem_ratio, args.ohem_min_kept, args.ohem_thresh) == (0.0, 1, 0.0)
    assert type(seg.build_criterion(args)) is BCEWithLogitsLoss          # the defaults build today's criteria
    assert type(seg.build_criterion(seg.parse_args(["--num_classes", "3"]))) is CrossEntropyLoss
    crit = seg.build_criterion(seg.parse_args(["--num_classes", "3", "--ohem_ratio", "0.25", "--ohem_thresh", "0.7"]))
    assert isinstance(crit, OHEMCrossEntropyLoss) and (crit.keep_ratio, crit.min_kept, crit.thresh) == (0.25, 1, 0.7)
    assert isinstance(seg.build_criterion(seg.parse_args(["--ohem_ratio", "0.1", "--ohem_min_kept", "9"])),
                      OHEMBCEWithLogitsLoss)
    for argv in (["--ohem_ratio", "0.25", "--loss", "ce+dice"], ["--ohem_ratio", "0.25", "--loss", "dice"],
                 ["--ohem_ratio", "1.5"], ["--ohem_ratio", "0.5", "--ohem_thresh", "1.0"]):
        with pytest.raises(SystemExit):
            seg.parse_args(argv)
