"""The classification cross-entropy kernels (csrc/kernels/cls_ce.hip) against the fp64 closed form (RefBackend
on the CPU), at the class counts where a row's split into an unaligned head, 16-byte pieces and a tail changes
(K = 2 .. 1000, one row per wave), with ignored and out-of-range labels on either side of a mixed target.

Tolerances are those of the pixel-wise loss for the same fp32 __expf / __logf arithmetic against fp64
(tests/test_pixel_ce_gpu.py): loss |d| < 1e-4, gradient relative L2 < 1e-4."""
import math
import os
import subprocess
import sys

import pytest
import torch

from deeplearning_mpi_amd.ops import backward, cross_entropy

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = [2, 10, 12, 63, 64, 65, 257, 1000]
MODES = ["hard", "lam0", "lam0.3", "lam1", "rows"]


def _labels(N, K, ignore_index, g):
    a = torch.randint(K, (N,), generator=g)
    b = torch.randint(K, (N,), generator=g)
    if N >= 5:
        a[0] = ignore_index                      # a ignored
        b[1] = ignore_index                      # b ignored
        a[2] = b[2] = ignore_index               # both ignored: m = 0
        a[3] = K + 3                             # out of range above
        b[4] = -1                                # out of range below
    return a, b


def _lam(mode, N, g):
    if mode == "hard":
        return None
    if mode == "rows":
        lam = torch.rand(N, generator=g)
        lam[::3] = 0.0
        lam[1::7] = 1.0
        return lam
    return torch.tensor([float(mode[3:])])


def _reference(x, a, b, lam, w, ignore_index, eps):
    """fp64 closed form on the CPU -> (loss, gradient)."""
    xd = x.double().requires_grad_(True)
    kw = {} if lam is None else dict(labels_b=b, lam=lam.double())
    loss = cross_entropy(xd, a, None if w is None else w.double(), ignore_index, eps, **kw)
    loss.backward()
    return loss.detach(), xd.grad


def _native(x, a, b, lam, w, ignore_index, eps):
    xg = x.to(DEV).requires_grad_(True)
    kw = {} if lam is None else dict(labels_b=b.to(DEV), lam=lam.to(DEV))
    loss = cross_entropy(xg, a.to(DEV), None if w is None else w.to(DEV), ignore_index, eps, **kw)
    backward(loss)
    return loss.detach().cpu(), xg.grad.cpu()


def _dead_rows(a, b, lam, K, ignore_index):
    """rows with m_n = 0"""
    keep = lambda y: ((y != ignore_index) & (y >= 0) & (y < K)).float()   # noqa: E731
    if lam is None:
        return keep(a) == 0
    lam = lam.expand(a.numel())
    return lam * keep(a) + (1 - lam) * keep(b) == 0


def _compare(x, a, b, lam, w, ignore_index, eps, what):
    K = x.shape[1]
    l0, g0 = _reference(x, a, b, lam, w, ignore_index, eps)
    l1, g1 = _native(x, a, b, lam, w, ignore_index, eps)
    dead = _dead_rows(a, b, lam, K, ignore_index)
    assert torch.equal(g1[dead], torch.zeros_like(g1[dead])), what
    if math.isnan(float(l0)):                     # nothing kept
        assert math.isnan(float(l1)) and torch.equal(g1, torch.zeros_like(g1)), what
        return
    assert abs(float(l0) - float(l1)) < 1e-4, (what, float(l0), float(l1))
    ref = float(g0.norm())
    if ref == 0:
        assert torch.equal(g1, torch.zeros_like(g1)), what
    else:
        assert float((g1.double() - g0).norm()) / ref < 1e-4, what


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
def test_against_fp64(K, mode):
    g = torch.Generator().manual_seed(1000 * K + MODES.index(mode))
    for N in (1, 5, 130):
        for eps in (0.0, 0.1):
            for weighted in (False, True):
                ignore_index = K - 1 if weighted else -100     # a custom in-range index with the weights
                x = torch.randn(N, K, generator=g) * 3
                a, b = _labels(N, K, ignore_index, g)
                w = torch.rand(K, generator=g) + 0.5 if weighted else None
                if mode == "hard" and eps == 0 and not weighted:
                    w = torch.ones(K)                          # every default would run the plain kernels
                _compare(x, a, b, _lam(mode, N, g), w, ignore_index, eps, (N, K, eps, weighted, mode))


@pytest.mark.parametrize("K", [10, 12, 65])
def test_logits_four_bytes_past_a_16_byte_boundary(K):
    g = torch.Generator().manual_seed(K)
    N = 7
    x = torch.randn(N, K, generator=g)
    a, b = _labels(N, K, -100, g)
    lam = torch.tensor([0.3], device=DEV)
    buf = torch.empty(N * K + 1, device=DEV)
    assert buf.data_ptr() % 16 == 0
    xg = buf[1:].view(N, K)
    xg.copy_(x)
    xg.requires_grad_(True)
    assert xg.data_ptr() % 16 == 4 and xg.is_contiguous()
    loss = cross_entropy(xg, a.to(DEV), label_smoothing=0.1, labels_b=b.to(DEV), lam=lam)
    backward(loss)
    l0, g0 = _reference(x, a, b, lam.cpu(), None, -100, 0.1)
    assert abs(float(l0) - float(loss)) < 1e-4
    assert float((xg.grad.cpu().double() - g0).norm() / g0.norm()) < 1e-4


def test_large_logits_stay_finite():
    """A row of +-80 next to one entry of 1e4.  With the label on the large entry the row's loss is ~0 and the
    bounds of this file hold as they are.  With label smoothing the same row's loss is ~1e3 (eps / K times the
    sum of lse - x_c ~ 1e4 each), where consecutive fp32 numbers are 6e-5 apart and the issue's own
    formulation lse * sum(w) - sum(w x) cancels at 1e5: there the result is checked to be finite and within
    1e-6 of the fp64 value relatively (16 fp32 roundings)."""
    g = torch.Generator().manual_seed(3)
    N, K = 5, 12
    x = torch.randn(N, K, generator=g)
    a = torch.randint(K, (N,), generator=g)
    x[1] = torch.tensor([80.0, -80.0] * (K // 2))
    x[1, int(a[1])] = 1e4
    w = torch.rand(K, generator=g) + 0.5
    _compare(x, a, a, None, w, -100, 0.0, "label on the large entry")
    l0, g0 = _reference(x, a, a, None, w, -100, 0.1)
    l1, g1 = _native(x, a, a, None, w, -100, 0.1)
    assert math.isfinite(float(l1)) and bool(torch.isfinite(g1).all())
    assert abs(float(l0) - float(l1)) < 1e-6 * abs(float(l0))
    assert float((g1.double() - g0).norm() / g0.norm()) < 1e-4


def test_all_rows_ignored():
    x = torch.randn(6, 10)
    a = torch.full((6,), -100)
    for kw in (dict(label_smoothing=0.1), dict(weight=torch.ones(10, device=DEV)),
               dict(labels_b=a.to(DEV), lam=torch.tensor([0.5], device=DEV))):
        xg = x.to(DEV).requires_grad_(True)
        loss = cross_entropy(xg, a.to(DEV), **kw)
        backward(loss)
        assert math.isnan(float(loss)) and torch.equal(xg.grad, torch.zeros_like(xg.grad))


def test_two_runs_are_bit_equal():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(130, 1000, generator=g)
    a, b = _labels(130, 1000, -100, g)
    lam, w = torch.rand(130, generator=g), torch.rand(1000, generator=g) + 0.5
    first = _native(x, a, b, lam, w, -100, 0.1)
    again = _native(x, a, b, lam, w, -100, 0.1)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_replayed_graph_follows_lam_and_labels():
    """tests/cls_ce_graph_replay.py in a process of its own: a capture creates HIP streams, and the streams this
    process has created so far decide which hardware queue a later test's streams share -- the negative control
    of tests/test_comm_ordering_gpu.py sees its race only on a queue of its own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "cls_ce_graph_replay.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "replays equal eager: 4" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
