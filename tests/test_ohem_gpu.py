"""Online hard example mining (csrc/kernels/ohem.hip) against the plain fp64 reference of tests/ohem_ref.py: loss,
gradient and the selected set in every kernel form, the radix select bit for bit at each level, ties and limits,
the grid-stride wrap, and determinism under graph replay (tests/ohem_graph_replay.py).

Tolerances are the plain pixel loss's own (tests/test_pixel_ce_gpu.py; the per-pixel arithmetic is the same):
loss |d| < 1e-4, gradient relative L2 < 1e-4; k, n_selected and the zeros outside S are exact."""
import math
import os
import subprocess
import sys

import pytest
import torch

import ohem_ref as R
from deeplearning_mpi_amd.ops import (OHEMBCEWithLogitsLoss, OHEMCrossEntropyLoss, cross_entropy, make_backend,
                                      ohem_cross_entropy)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _layout(x, layout):   # class-last CPU storage -> device [N, K, H, W]
    x = x.to(DEV).permute(0, 3, 1, 2)
    return x if layout == "nhwc_view" else x.contiguous()


def _check(crit, x, target, ref, what):
    loss = crit(x, target)
    (gx,) = torch.autograd.grad(loss, x)
    lr, gr, sel, k = ref
    st = {n: v.item() for n, v in crit.last_stats.items()}
    dl, dg = abs(loss.item() - lr.item()), R.rel_l2(gx, gr)
    print(f"{what}: loss |d| {dl:.3e}, grad rel L2 {dg:.3e}, k {st['k']}/{k}, n_selected {st['n_selected']}/{sel.sum()}")
    assert dl < 1e-4 and dg < 1e-4
    assert st["k"] == k and st["n_selected"] == sel.sum().item()
    assert gx.stride() == x.stride() and gx.dtype == torch.float32
    off = ~sel.to(DEV)
    assert (gx.reshape(sel.shape[0], -1, *sel.shape[1:]).permute(0, 2, 3, 1)[off] == 0).all()   # exact zeros off S


@pytest.mark.parametrize("setting", R.SETTINGS, ids=str)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("K", [2, 3, 4, 5, 21, 40])   # registers (vector forms at 2, 4), online (nchw), LDS tiles
def test_softmax_loss_and_gradient_match_fp64(K, layout, weighted, setting):
    xc, y, w = R.softmax_inputs(K, R.SEEDS[K])
    x = _layout(xc, layout).requires_grad_(True)
    w = w if weighted else None
    crit = OHEMCrossEntropyLoss(weight=w, keep_ratio=setting[0], min_kept=setting[1], thresh=setting[2]).to(DEV)
    _check(crit, x, y.to(DEV), R.softmax_reference(x.cpu(), y, w, *setting), f"K={K} {layout} w={weighted} {setting}")


@pytest.mark.parametrize("setting", R.SETTINGS, ids=str)
@pytest.mark.parametrize("kind", ["hard", "soft"])
@pytest.mark.parametrize("channel", [False, True])
def test_binary_loss_and_gradient_match_fp64(channel, kind, setting):
    xc, t = R.binary_inputs(kind, R.SEEDS[kind])
    x = (xc.unsqueeze(1) if channel else xc).to(DEV).requires_grad_(True)
    crit = OHEMBCEWithLogitsLoss(keep_ratio=setting[0], min_kept=setting[1], thresh=setting[2])
    _check(crit, x, t.to(DEV), R.binary_reference(xc, t, *setting), f"binary channel={channel} {kind} {setting}")


def _pattern(name):
    """70,001 fp32 bit patterns (more than 256 blocks' worth of lanes, odd) in which one level of the select decides."""
    g = torch.Generator().manual_seed(7)
    n = 70001
    r = torch.randint(0, 2 ** 31 - 1, (n,), generator=g)
    if name == "low":
        bits = 0x3F800000 | (r & 0x1FF)          # differ in bits 8..0 only
    elif name == "mid":
        bits = 0x3F800000 | (r & 0xFFE00)        # differ in bits 19..9 only
    elif name == "top":
        bits = (r % 2000 + 24) << 20             # differ in bits 30..20 only, finite
    else:
        bits = torch.rand(n, generator=g).view(torch.int32).long()
        cover = torch.rand(n, generator=g)
        if name == "zeros":
            bits[cover < 0.6] = 0
        else:
            bits[cover < 0.3] = 0xBF800000 - 2 ** 32   # -1: not valid
    return bits.to(torch.int32).view(torch.float32)


@pytest.mark.parametrize("rank", [1, 2, -1, 0, "ratio"])   # k = 1, 2, n_valid - 1, n_valid, ceil(0.37 n_valid)
@pytest.mark.parametrize("name", ["low", "mid", "top", "zeros", "sentinel"])
def test_selection_is_exact(name, rank):
    v = _pattern(name)
    dv = v.to(DEV)
    if name == "mid":   # from 4 bytes past a 16-byte boundary: a partial 16-byte group at either end
        v, dv = v[1:], dv[1:]
    valid = v.view(torch.int32) >= 0
    srt = v[valid].sort(descending=True).values
    nv = srt.numel()
    k = math.ceil(0.37 * nv) if rank == "ratio" else rank if rank > 0 else nv + rank
    st = make_backend(DEV).ohem_select(dv, *((0.37, 1) if rank == "ratio" else (1e-9, k)))
    cut = srt[k - 1]
    assert st["k"].item() == k and st["n_valid"].item() == nv
    assert st["cut"].cpu().view(torch.int32).item() == cut.view(torch.int32).item()   # bit-equal
    assert st["n_selected"].item() == (valid & (v >= cut)).sum().item()


def test_ties_are_all_selected():
    xc, y, _ = R.softmax_inputs(3, 11, (1, R.H, R.W))
    x = _layout(torch.cat([xc, xc]), "nhwc_view").requires_grad_(True)
    crit = OHEMCrossEntropyLoss(keep_ratio=1e-9, min_kept=101)
    (gx,) = torch.autograd.grad(crit(x, torch.cat([y, y]).to(DEV)), x)
    assert crit.last_stats["k"].item() == 101 and crit.last_stats["n_selected"].item() == 102
    assert torch.equal(gx[0], gx[1]) and gx.abs().sum() > 0


def test_limits():
    xc, y, w = R.softmax_inputs(5, 3)
    x, y, w = _layout(xc, "nhwc_view").requires_grad_(True), y.to(DEV), w.to(DEV)
    full = ohem_cross_entropy(x, y, weight=w, keep_ratio=1.0, min_kept=1)
    plain = cross_entropy(x, y, weight=w)
    assert abs(full.item() - plain.item()) < 1e-6
    assert R.rel_l2(torch.autograd.grad(full, x)[0], torch.autograd.grad(plain, x)[0]) < 1e-6
    crit = OHEMCrossEntropyLoss(keep_ratio=0.01, min_kept=10 ** 6)   # min_kept > n_valid: every valid pixel
    crit(x, y)
    assert crit.last_stats["n_selected"].item() == crit.last_stats["n_valid"].item() == ((y >= 0) & (y < 5)).sum().item()
    loss = ohem_cross_entropy(x, torch.full_like(y, -100))
    assert torch.isnan(loss) and (torch.autograd.grad(loss, x)[0] == 0).all()


def test_grid_stride_wrap():
    """547,600 pixels: more than 2048 blocks of 256, so the forward's loop runs twice."""
    xc, y, _ = R.softmax_inputs(2, R.SEEDS["wrap"], (1, 740, 740))
    x = _layout(xc, "nhwc_view").requires_grad_(True)
    _check(OHEMCrossEntropyLoss(keep_ratio=0.01), x, y.to(DEV), R.softmax_reference(x.cpu(), y, None, 0.01, 1, None),
           "740 x 740")


def test_deterministic_and_follows_inputs_under_replay():
    """tests/ohem_graph_replay.py in a process of its own (as tests/test_cls_ce_gpu.py's replay test)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "ohem_graph_replay.py")], cwd=root,
                       env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "replays equal eager: 2" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
