"""The fp64 reference of tests/optim_ref.py against independent derivations on the CPU: torch.optim.SGD,
Adam and AdamW stepping fp64 parameters for 25 updates, clip_grad_norm_'s scaling, RefBackend.cast_weights
and Tensor.to(bfloat16) on every bf16 rounding case, all exact or at 1e-12 relative.  The GPU tests hold the
HIP kernels to optim_ref; this file holds optim_ref to torch."""
import itertools
import math

import pytest
import torch

import optim_ref as R
from deeplearning_mpi_amd.ops.backend import RefBackend

F64 = torch.float64
TOL = 1e-12
STEPS = 25
N = 257


def _close(a, b):
    scale = b.abs().max().item()
    return (a - b).abs().max().item() <= TOL * max(scale, 1e-300)


def _grads(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, dtype=F64, generator=g) * (1 + k % 3) for k in range(STEPS)]


@pytest.mark.parametrize("momentum,dampening,wd,nesterov",
                         [(m, d, w, n) for m, d, w, n in itertools.product((0.0, 0.9), (0.0, 0.1), (0.0, 1e-4),
                                                                           (False, True))
                          if not (n and (m == 0 or d != 0))])   # torch refuses nesterov with those
def test_sgd_matches_torch(momentum, dampening, wd, nesterov):
    """25 updates, the first with the first-step rule (momentum buffer = d, no dampening)."""
    grads = _grads(1)
    p0 = torch.randn(N, dtype=F64, generator=torch.Generator().manual_seed(2))
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([tp], lr=0.05, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    p, m = p0.clone(), torch.full_like(p0, 123.0)   # the first step must not read m
    for k, g in enumerate(grads):
        tp.grad = g.clone()
        opt.step()
        m_in = m
        p, m = R.sgd(p, g, m, 0.05, momentum, dampening, wd, nesterov, k == 0)
        if momentum == 0:
            assert m is m_in or torch.equal(m, m_in)
        assert _close(p, tp.detach()), k
    if momentum != 0:
        assert _close(m, opt.state[tp]["momentum_buffer"])


def test_sgd_skip_and_momentum_zero_rules():
    p, g, m = torch.randn(9, dtype=F64), torch.randn(9, dtype=F64), torch.randn(9, dtype=F64)
    for s in (1.0, -3.0, float("nan"), torch.tensor([float("nan")]), torch.tensor([2.0])):
        p2, m2 = R.sgd(p, g, m, 0.1, 0.9, 0.0, 1e-4, True, False, skip=s)
        assert torch.equal(p2, p) and torch.equal(m2, m)
    for s in (None, 0.0, -0.0, torch.tensor([-0.0])):
        p2, m2 = R.sgd(p, g, m, 0.1, 0.9, 0.0, 0.0, False, False, skip=s)
        assert torch.equal(m2, 0.9 * m + g) and torch.equal(p2, p - 0.1 * m2)
    p2, m2 = R.sgd(p, g, m, 0.1, 0.0, 0.5, 0.0, True, True)   # momentum 0: m stays, nesterov / dampening unused
    assert torch.equal(m2, m) and torch.equal(p2, p - 0.1 * g)
    # nesterov is not coupled to dampening (torch refuses the pair; the kernels define it)
    p2, m2 = R.sgd(p, g, m, 0.1, 0.9, 0.1, 0.0, True, False)
    assert torch.equal(m2, 0.9 * m + (1 - 0.1) * g) and torch.equal(p2, p - 0.1 * (g + 0.9 * m2))


@pytest.mark.parametrize("cls,wd", [(torch.optim.Adam, 0.0), (torch.optim.Adam, 1e-2), (torch.optim.AdamW, 0.0),
                                    (torch.optim.AdamW, 1e-2)])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)])
def test_adam_matches_torch(cls, wd, betas):
    grads = _grads(3)
    p0 = torch.randn(N, dtype=F64, generator=torch.Generator().manual_seed(4))
    tp = torch.nn.Parameter(p0.clone())
    opt = cls([tp], lr=1e-2, betas=betas, eps=1e-8, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for k, g in enumerate(grads):
        tp.grad = g.clone()
        opt.step()
        p, g2, m, v = R.adam(p, g, m, v, 1e-2, betas[0], betas[1], 1e-8, wd, cls is torch.optim.AdamW, k + 1)
        assert torch.equal(g2, g)
        assert _close(p, tp.detach()), k
    assert _close(m, opt.state[tp]["exp_avg"]) and _close(v, opt.state[tp]["exp_avg_sq"])


def test_adam_bias_corrections_come_from_bc_betas():
    """Moments from the fp32-rounded betas, corrections from the doubles: equal to a step whose corrections are
    handed over explicitly, different from one that derives them from the rounded betas."""
    g = torch.randn(33, dtype=F64)
    p, z = torch.randn(33, dtype=F64), torch.zeros(33, dtype=F64)
    b1, b2 = R.f32(0.9), R.f32(0.999)
    assert b2 != 0.999
    for t in (1, 2, 1000):
        pa, _, ma, va, d = R.adam(p, g, z, z, 1e-3, b1, b2, 1e-8, 0.0, False, t, bc_betas=(0.9, 0.999), detail=True)
        assert d["bc1"] == 1 - 0.9 ** t and d["bc2"] == 1 - 0.999 ** t
        m = z + (g - z) * (1 - b1)
        v = z * b2 + (1 - b2) * g * g
        want = p - (1e-3 / (1 - 0.9 ** t)) * m / (v.sqrt() / math.sqrt(1 - 0.999 ** t) + 1e-8)
        assert torch.equal(ma, m) and torch.equal(va, v) and _close(pa, want)
        pb = R.adam(p, g, z, z, 1e-3, b1, b2, 1e-8, 0.0, False, t)[0]
        assert not _close(pb, want)   # 1 - fl32(0.999)^t is 1e-5 off: the deviation the kernels must not have


def test_adam_coef_writeback_skip():
    g = torch.randn(17, dtype=F64)
    p, m, v = torch.randn(17, dtype=F64), torch.randn(17, dtype=F64), torch.rand(17, dtype=F64)
    a = R.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, False, 3, coef=0.5, writeback=True)
    b = R.adam(p, g * 0.5, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, False, 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))            # clip, then the step; g is the clipped one
    assert torch.equal(R.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, 3, coef=0.5)[1], g)
    assert torch.equal(R.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, 3, coef=1.0, writeback=True)[1], g)
    for s in (1.0, float("nan")):
        out = R.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, 3, coef=0.5, skip=s, writeback=True)
        assert all(torch.equal(x, y) for x, y in zip(out, (p, g, m, v)))


@pytest.mark.parametrize("scale", [0.01, 1.0, 30.0])
def test_grad_norm_matches_clip_grad_norm(scale):
    gs = [torch.randn(n, dtype=F64, generator=torch.Generator().manual_seed(n)) * scale for n in (5, 64, 257)]
    flat = torch.cat(gs)
    for max_norm in (0.5, float(flat.norm()), 1e3):
        ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
        for q, g in zip(ps, gs):
            q.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        norm, coef, bad = R.grad_norm(flat, max_norm)
        assert bad == 0.0 and abs(norm - float(total)) <= TOL * norm
        assert _close(flat * coef, torch.cat([q.grad for q in ps]))
    inf, nan = flat.clone(), flat.clone()
    inf[7], nan[9] = float("inf"), float("nan")
    assert R.grad_norm(inf, 1.0)[1:] == (0.0, 1.0) and R.grad_norm(-inf, 1.0)[1:] == (0.0, 1.0)
    n, c, f = R.grad_norm(nan, 1.0)
    assert math.isnan(n) and (c, f) == (1.0, 1.0)


RELAYOUTS = [  # dims, valid, strides of a source that holds them
    ([4, 3, 3, 8], [4, 3, 3, 5], [45, 15, 5, 1]),           # channel padding
    ([16, 1, 1, 24], [16, 1, 1, 24], [1, 0, 0, 16]),        # transpose
    ([5, 2, 2, 7], [3, 2, 1, 7], [1, 21, 3, 42]),           # short in every dim but one
    ([2, 2, 2, 4], [2, 2, 2, 4], [16, 8, 4, 1]),            # identity
]


@pytest.mark.parametrize("dims,valid,strides", RELAYOUTS)
def test_relayout_matches_refbackend(dims, valid, strides):
    need = 1 + sum((v - 1) * s for v, s in zip(valid, strides))
    src = torch.randn(need + 3, generator=torch.Generator().manual_seed(need))[1:1 + need]
    n = dims[0] * dims[1] * dims[2] * dims[3]
    flat = torch.full((n + 10,), 7.0)
    RefBackend("cpu").cast_weights([(src, 5, dims, valid, strides)], n + 10, flat)
    got = R.relayout(src, dims, valid, strides)
    assert torch.equal(got.reshape(-1), flat[5:5 + n]) and got.dtype == torch.float32


@pytest.mark.parametrize("low", [0x0000, 0x7fff, 0x8000, 0x8001])
def test_bf16_rounding_matches_torch_on_every_pattern(low):
    """All 65536 high halves: ties to even (0x8000 after an even / odd kept bit), the carry into the exponent,
    the largest finite bf16 plus half an ulp -> inf, denormals, infinities; NaNs compared as NaNs."""
    bits = (torch.arange(65536, dtype=torch.int64) << 16) | low
    x = bits.to(torch.int32).view(torch.float32)
    want = x.to(torch.bfloat16)
    got = R.bf16_bits(x)
    wbits = want.view(torch.int16).to(torch.int32) & 0xffff
    nan = x.isnan()
    assert int(nan.sum()) == (2 * 127 if low == 0 else 2 * 128)
    assert torch.equal(got[~nan], wbits[~nan])
    g = (got << 16).view(torch.float32)
    assert bool(g[nan].isnan().all()) and bool(want[nan].isnan().all())
    assert torch.equal(R.bf16_round(x)[~nan], want.float()[~nan])
    if low == 0x8000:
        i = 0x7f7f   # the largest finite bf16 plus half an ulp
        assert got[i] == 0x7f80 and got[0x3f80] == 0x3f80 and got[0x3f81] == 0x3f82   # ties: to even


def test_gather_reference():
    src = torch.arange(10.0) + 1
    idx = torch.tensor([3, -1, 3, 0, 9, -7])
    dst = torch.full((8,), 100.0)
    assert R.gather(dst, src, idx).tolist() == [4, 0, 4, 1, 10, 0, 100, 100]
    assert R.gather(dst, src, idx, True).tolist() == [104, 100, 104, 101, 110, 100, 100, 100]
    assert dst.tolist() == [100.0] * 8
    rb = dst.clone()
    RefBackend("cpu").gather_(rb, src, idx, True)
    assert torch.equal(rb, R.gather(dst, src, idx, True))
