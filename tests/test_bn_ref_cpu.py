"""The fp64 BatchNorm reference of tests/bn_ref.py against an independent derivation: torch autograd
through torch.nn.functional.batch_norm(training=True) + relu, in fp64.  The GPU tests hold the HIP
kernels to bn_ref; this file holds bn_ref to torch."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

N, H, W = 2, 5, 7
EPS, MOM = 1e-5, 0.1


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _case(C, seed):
    g = torch.Generator().manual_seed(seed)
    M = N * H * W
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rnd(M, C) * 2.0 + rnd(C) * 3.0
    res = rnd(M, C)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, rnd(C)
    dy = rnd(M, C)
    rm, rv = rnd(C), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return x, res, gamma, beta, dy, rm, rv


def _nchw(t, C):
    return t.reshape(N, H, W, C).permute(0, 3, 1, 2)


def _rows(t, C):
    return t.permute(0, 2, 3, 1).reshape(-1, C)


@pytest.mark.parametrize("C", [24, 192])
def test_composition_matches_autograd(C):
    x, res, gamma, beta, dy, rm, rv = _case(C, C)
    M = N * H * W
    # torch: y = relu(BN_train(x) + res), gradients by autograd
    xt, rt = _nchw(x, C).clone().requires_grad_(), _nchw(res, C).clone().requires_grad_()
    gt, bt = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    rmt, rvt = rm.clone(), rv.clone()
    pre_t = F.batch_norm(xt, rmt, rvt, gt, bt, True, MOM, EPS) + rt
    yt = torch.relu(pre_t)
    yt.backward(_nchw(dy, C))
    # no pre-activation near zero: relu's derivative at 0 and the stored-y mask cannot disagree
    assert pre_t.detach().abs().min().item() > 1e-6

    # bn_ref, stage by stage
    s1, s2 = R.sums(x)
    f = R.fwd_finalize(s1, s2, M, gamma, beta, EPS, rm, rv, MOM)
    y = R.apply(x, f["scale"], f["shift"], res, relu=True)
    b1, b2 = R.bwd_reduce(dy, y, x, f["mean"], f["invstd"])
    k = R.bwd_finalize(b1, b2, M, gamma, f["mean"], f["invstd"], torch.zeros(C), torch.zeros(C))
    dyr = R.masked(dy, y)
    dx = R.bwd_apply(dyr, x, k["k1"], k["k2"], k["k3"])

    tol = 1e-10
    assert _rel(y, _rows(yt.detach(), C)) < tol
    assert _rel(f["running_mean"], rmt) < tol
    assert _rel(f["running_var"], rvt) < tol
    assert _rel(dx, _rows(xt.grad, C)) < tol
    assert _rel(dyr, _rows(rt.grad, C)) < tol           # dres: the masked gradient
    assert _rel(k["dgamma"], gt.grad) < tol
    assert _rel(k["dbeta"], bt.grad) < tol
    # the mask bits say the same as y > 0
    bits = R.mask_bits(y)
    e = torch.arange(8)
    unpacked = ((bits.to(torch.int32).unsqueeze(-1) >> e) & 1).reshape(M, C).bool()
    assert torch.equal(unpacked, y > 0)


@pytest.mark.parametrize("C", [24, 192])
def test_raw_z_form_equals_xhat_form(C):
    x, res, gamma, beta, dy, _, _ = _case(C, 100 + C)
    f = R.fwd_finalize(*R.sums(x), N * H * W, gamma, beta, EPS)
    y = R.apply(x, f["scale"], f["shift"], res)
    a1, a2 = R.bwd_reduce(dy, y, x, f["mean"], f["invstd"])
    b1, b2, _ = R.bwd_reduce_raw(dy, y, x, f["mean"], f["invstd"])
    assert torch.equal(a1, b1)
    assert _rel(b2, a2) < 1e-10


def test_affine_residual_and_no_affine():
    """The Deferred.bn residual (res*rscale + rshift) and gamma / beta = None against plain torch."""
    C = 24
    x, res, gamma, beta, _, _, _ = _case(C, 7)
    f = R.fwd_finalize(*R.sums(x), N * H * W, None, None, EPS)
    bn = F.batch_norm(_nchw(x, C), None, None, None, None, True, MOM, EPS)
    y = R.apply(x, f["scale"], f["shift"], res, gamma, beta, relu=False)
    assert _rel(y, _rows(bn, C) + res * gamma + beta) < 1e-10
    k = R.bwd_finalize(torch.ones(C), torch.ones(C), 5, None, f["mean"], f["invstd"])
    assert torch.equal(k["k1"], f["invstd"]) and "dgamma" not in k


def test_count_one_and_constant_channel_are_finite():
    C = 8
    x = torch.randn(1, C, dtype=torch.float64)
    f = R.fwd_finalize(*R.sums(x), 1, None, None, EPS, torch.zeros(C), torch.ones(C), MOM)
    for v in f.values():
        assert torch.isfinite(v).all()
    assert torch.equal(f["unbiased"], f["var"])          # count == 1: no n / (n - 1)
    assert f["var"].abs().max().item() < 1e-12
    x = torch.randn(35, C, dtype=torch.float64)
    x[:, 3] = 1.5                                        # a constant channel: zero variance
    dy = torch.randn(35, C, dtype=torch.float64)
    f = R.fwd_finalize(*R.sums(x), 35, None, None, EPS)
    assert f["var"][3].item() == 0.0 and f["invstd"][3].item() == pytest.approx(EPS ** -0.5, rel=1e-12)
    b1, b2 = R.bwd_reduce(dy, None, x, f["mean"], f["invstd"])
    k = R.bwd_finalize(b1, b2, 35, None, f["mean"], f["invstd"], torch.zeros(C), torch.zeros(C))
    dx = R.bwd_apply(dy, x, k["k1"], k["k2"], k["k3"])
    assert all(torch.isfinite(v).all() for v in k.values()) and torch.isfinite(dx).all()


def test_half_ulp_bf16():
    ref = torch.tensor([1.0, 1.5, 1.999, 2.0, -3.0, 2.0 ** -100, 0.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -108, 0.0], dtype=torch.float64)
    assert torch.equal(R.half_ulp_bf16(ref), want)
    # the nearest bf16 of any value lies within it
    v = torch.randn(10000, dtype=torch.float64) * 5
    assert bool(((v.to(torch.bfloat16).double() - v).abs() <= R.half_ulp_bf16(v)).all())
