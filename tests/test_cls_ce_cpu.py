"""The classification cross-entropy with weight / ignore_index / label smoothing and two-label mixed targets
(ops/losses.py cross_entropy on [N, K] logits), without a GPU: the closed form of RefBackend in fp64 against
torch, the mixed-target identity, the corner cases, and the binder's argument rules through their integer-only
binding (csrc/binding/loss.cpp check_cls_ce_args) -- one refused call per rule."""
import math

import pytest
import torch
import torch.nn.functional as F

from deeplearning_mpi_amd import ops
from deeplearning_mpi_amd._ext import native
from deeplearning_mpi_amd.ops.losses import _CE


def _case(N=9, K=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, K, generator=g, dtype=torch.float64) * 3
    a = torch.randint(K, (N,), generator=g)
    b = torch.randint(K, (N,), generator=g)
    w = torch.rand(K, generator=g, dtype=torch.float64) + 0.5
    return x, a, b, w


def _ours(x, a, **kw):
    x = x.clone().requires_grad_(True)
    loss = ops.cross_entropy(x, a, **kw)
    loss.backward()
    return loss.detach(), x.grad


def _torch(x, a, **kw):
    x = x.clone().requires_grad_(True)
    loss = F.cross_entropy(x, a, **kw)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.4])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ignore_index", [-100, 3])
def test_matches_torch_in_fp64(eps, weighted, ignore_index):
    x, a, _, w = _case()
    a[2] = ignore_index
    if eps == 0 and not weighted and ignore_index == -100:
        a[2] = 1                      # every default would go to the plain kernels: covered below
        eps_kw = dict(weight=torch.ones(7, dtype=torch.float64))
    else:
        eps_kw = dict(weight=w if weighted else None)
    l0, g0 = _torch(x, a, ignore_index=ignore_index, label_smoothing=eps, **eps_kw)
    l1, g1 = _ours(x, a, ignore_index=ignore_index, label_smoothing=eps, **eps_kw)
    assert abs(float(l0 - l1)) < 1e-13
    assert float((g0 - g1).abs().max()) < 1e-13


def test_out_of_range_labels_are_ignored():
    x, a, _, w = _case()
    a2 = a.clone()
    a[1], a[4] = 7 + 3, -1
    a2[1], a2[4] = -100, -100
    l0, g0 = _torch(x, a2, weight=w, label_smoothing=0.1)
    l1, g1 = _ours(x, a, weight=w, label_smoothing=0.1)
    assert abs(float(l0 - l1)) < 1e-13 and float((g0 - g1).abs().max()) < 1e-13
    assert torch.equal(g1[1], torch.zeros(7, dtype=torch.float64)) and torch.equal(g1[4], g1[1])


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_scalar_lam_identity(lam, eps):
    """no weight, nothing ignored: lam CE(x, a) + (1 - lam) CE(x, b), each term smoothed."""
    x, a, b, _ = _case()
    la, ga = _torch(x, a, label_smoothing=eps)
    lb, gb = _torch(x, b, label_smoothing=eps)
    l1, g1 = _ours(x, a, label_smoothing=eps, labels_b=b, lam=torch.tensor([lam], dtype=torch.float64))
    assert abs(float(lam * la + (1 - lam) * lb - l1)) < 1e-13
    assert float((lam * ga + (1 - lam) * gb - g1).abs().max()) < 1e-13


def test_per_row_lam_gradient_matches_autograd():
    x, a, b, w = _case()
    b[3], a[5] = -100, -100
    a[6] = b[6] = -100
    lam = torch.rand(9, dtype=torch.float64)
    eps, K = 0.1, 7
    xr = x.clone().requires_grad_(True)
    keep_a, keep_b = (a != -100).double(), (b != -100).double()
    t = (lam * keep_a)[:, None] * F.one_hot(a.clamp(0), K) + ((1 - lam) * keep_b)[:, None] * F.one_hot(b.clamp(0), K)
    m = lam * keep_a + (1 - lam) * keep_b
    q = (1 - eps) * t + eps / K * m[:, None]
    ref = -(w * q * torch.log_softmax(xr, 1)).sum() / (w * t).sum()
    ref.backward()
    l1, g1 = _ours(x, a, weight=w, label_smoothing=eps, labels_b=b, lam=lam)
    assert abs(float(ref.detach() - l1)) < 1e-13
    assert float((xr.grad - g1).abs().max()) < 1e-13
    assert torch.equal(g1[6], torch.zeros(K, dtype=torch.float64))


def test_nothing_kept_is_nan_with_a_zero_gradient():
    x, a, _, _ = _case()
    a[:] = -100
    l1, g1 = _ours(x, a, label_smoothing=0.1)
    assert math.isnan(float(l1))
    assert torch.equal(g1, torch.zeros_like(g1))


def test_pixelwise_logits_refuse_the_classification_arguments():
    x = torch.randn(2, 3, 4, 4)
    y = torch.randint(3, (2, 4, 4))
    with pytest.raises(NotImplementedError, match="pixel-wise"):
        ops.cross_entropy(x, y, label_smoothing=0.1)
    with pytest.raises(NotImplementedError, match="pixel-wise"):
        ops.cross_entropy(x, y, labels_b=y, lam=torch.ones(1))
    assert torch.isfinite(ops.CrossEntropyLoss()(x, y))   # the pixel-wise loss itself is as before


def test_labels_b_and_lam_come_together():
    x, a, b, _ = _case()
    with pytest.raises(ValueError, match="come together"):
        ops.cross_entropy(x, a, labels_b=b)
    with pytest.raises(ValueError, match="come together"):
        ops.cross_entropy(x, a, lam=torch.ones(1, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ops.cross_entropy(x, a, label_smoothing=1.0)
    with pytest.raises(ValueError, match="1 or N"):
        ops.cross_entropy(x, a, labels_b=b, lam=torch.ones(4, dtype=torch.float64))


def test_default_call_is_the_plain_loss():
    x, a, _, _ = _case()
    x = x.float()
    assert torch.equal(ops.cross_entropy(x, a), _CE.apply(x, a))
    assert torch.equal(ops.CrossEntropyLoss()(x, a), _CE.apply(x, a))
    crit = ops.CrossEntropyLoss(label_smoothing=0.1)
    assert abs(float(crit(x, a) - F.cross_entropy(x, a, label_smoothing=0.1))) < 1e-5


# ------------------------------------------------------------------ the binder's argument rules
C = native()
GOOD = dict(N=5, K=10, ldl=12, logits_numel=4 * 12 + 10, labels_numel=5, labels_b_numel=5, lam_numel=5, weight_numel=10,
            eps=0.1, lse_numel=5, rows_numel=15, den_numel=1)
BWD = dict(GOOD, fn="cls_ce_bwd", dlogits_numel=50, go_numel=1)
# what is refused, and a piece of the message of the rule it is meant to trip
REFUSED = {
    "N=0": (dict(N=0), "N must be >= 1"),
    "K=0": (dict(K=0), "K must be >= 1"),
    "logits not fp32": (dict(logits_f32=False), "logits must be fp32"),
    "ldl<K": (dict(ldl=9), "row stride"),
    "logits short by one": (dict(logits_numel=4 * 12 + 9), "logits shorter than"),
    "labels not int64": (dict(labels_i64=False), "labels must be int64"),
    "labels_b not int64": (dict(labels_b_i64=False), "labels must be int64"),
    "labels numel": (dict(labels_numel=4), "labels must have N"),
    "labels_b numel": (dict(labels_b_numel=6), "labels_b must have N"),
    "labels_b alone": (dict(lam_numel=-1), "come together"),
    "lam alone": (dict(labels_b_numel=-1), "come together"),
    "lam not fp32": (dict(lam_f32=False), "lam must be fp32"),
    "lam numel": (dict(lam_numel=2), "lam must have 1 or N"),
    "weight not fp32": (dict(weight_f32=False), "weight must be fp32"),
    "weight numel": (dict(weight_numel=12), "weight must have K"),
    "eps nan": (dict(eps=float("nan")), "finite"),
    "eps inf": (dict(eps=float("inf")), "finite"),
    "eps=1": (dict(eps=1.0), "[0, 1)"),
    "eps<0": (dict(eps=-0.1), "[0, 1)"),
    "lse numel": (dict(lse_numel=4), "lse must have N"),
    "rows numel": (dict(rows_numel=5), "rows must have 3 N"),
    "den numel": (dict(den_numel=2), "den must have 1"),
}
REFUSED_BWD = {
    "dlogits numel": (dict(dlogits_numel=5 * 12), "dlogits must have N K"),
    "go numel": (dict(go_numel=2), "go must have 1"),
}


def test_good_calls():
    assert C.cls_ce_check(**GOOD) == ""
    assert C.cls_ce_check(**BWD) == ""
    assert C.cls_ce_check(**{**GOOD, "lam_numel": 1}) == ""
    assert C.cls_ce_check(**{**GOOD, "eps": 0.0, "weight_numel": -1, "labels_b_numel": -1, "lam_numel": -1}) == ""
    assert C.cls_ce_check(N=1, K=1, ldl=1, logits_numel=1, labels_numel=1, lse_numel=1, rows_numel=3) == ""


@pytest.mark.parametrize("what", list(REFUSED))
def test_forward_refuses(what):
    change, piece = REFUSED[what]
    msg = C.cls_ce_check(**{**GOOD, **change})
    assert msg.startswith("cls_ce_fwd: ") and piece in msg, (what, msg)


@pytest.mark.parametrize("what", list(REFUSED) + list(REFUSED_BWD))
def test_backward_refuses(what):
    change, piece = {**REFUSED, **REFUSED_BWD}[what]
    msg = C.cls_ce_check(**{**BWD, **change})
    assert msg.startswith("cls_ce_bwd: ") and piece in msg, (what, msg)
