"""Data gradient of the K-class (K = 2..4) 1x1 UNet head as a streaming kernel (head.hip
head_dgrad_bn_kernel) against an fp64 reference on the same inputs: identical ReLU-mask decisions,
every stored dx within one bf16 ulp of the rounded fp64 value, BN-backward partials equal to the sums
of the stored dx; fp32 activations once; and a training UNet(out_classes=3) runs it.

The BN scale / shift (and z in the fp32 case) are bf16-representable values, so z * scale is exact in fp32
and fused and unfused evaluations of z * scale + shift > 0 agree bit for bit: the mask is unambiguous."""
import pytest
import torch

from deeplearning_mpi_amd.models.engine import BwdFuse
from deeplearning_mpi_amd.ops.act import Act
from deeplearning_mpi_amd.ops.backend import NativeBackend

pytestmark = pytest.mark.gpu
DEV = "cuda"
KP = 8


def _inputs(K, C, M, dtype):
    g = torch.Generator(device=DEV).manual_seed(K * 1000 + C + M)
    bf = lambda t: t.to(torch.bfloat16)   # noqa: E731
    dl = torch.zeros(M, KP, device=DEV, dtype=dtype)
    dl[:, :K] = bf(torch.randn(M, K, device=DEV, generator=g)).to(dtype)
    w = torch.zeros(C, KP, device=DEV, dtype=dtype)
    w[:, :K] = bf(torch.randn(C, K, device=DEV, generator=g) * 0.2).to(dtype)
    z = bf(torch.randn(M, C, device=DEV, generator=g)).to(dtype)
    sc = bf(torch.rand(C, device=DEV, generator=g) + 0.5).float()
    sh = bf(torch.randn(C, device=DEV, generator=g) * 0.3).float()
    return dl, w, z, sc, sh


def _run(be, K, C, M, dl, w, z, sc, sh):
    dx = torch.full((M, C), float("nan"), device=DEV, dtype=dl.dtype)
    part = be.head_dgrad_bn(Act(dl, 1, 1, M, KP), K, w.view(-1), KP, Act(dx, 1, 1, M, C),
                            BwdFuse(None, Act(z, 1, 1, M, C), None, sc, sh))
    torch.cuda.synchronize()
    return dx, part


def _reference(K, dl, w, z, sc, sh):
    keep32 = z.float() * sc + sh > 0
    keep64 = z.double() * sc.double() + sh.double() > 0
    assert torch.equal(keep32, keep64)   # the mask of these inputs does not depend on how it is evaluated
    full = dl[:, :K].double() @ w[:, :K].double().t()
    return keep64, full, full * keep64


def _check_partials(part, dx, z, C):
    assert part.dim() == 3 and part.shape[1:] == (2, C)
    ps = part.double().sum(0)
    v = dx.double()
    for got, terms in ((ps[0], v), (ps[1], v * z.double())):
        err = (got - terms.sum(0)).abs()
        bound = 1e-5 * terms.abs().sum(0)
        assert (err <= bound).all(), (err.max().item(), bound.min().item())
        ref = terms.sum(0)   # and norm-wise over the channels, relative to the sums themselves
        assert ((got - ref).norm() / ref.norm()).item() < 1e-5


@pytest.mark.parametrize("M", [257, 4096])   # 257: one row past a block multiple of the C = 64 row map
@pytest.mark.parametrize("C", [64, 16])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_head_dgrad_bn_bf16(K, C, M):
    be = NativeBackend(DEV)
    dl, w, z, sc, sh = _inputs(K, C, M, torch.bfloat16)
    dx, part = _run(be, K, C, M, dl, w, z, sc, sh)
    keep, full, ref = _reference(K, dl, w, z, sc, sh)
    assert torch.isfinite(dx).all()
    assert (dx[~keep] == 0).all()
    assert torch.equal((dx != 0) | (full == 0) | ~keep, torch.ones_like(keep))   # kept elements are written
    ref_bf = ref.to(torch.bfloat16).double()
    ulp = torch.ldexp(torch.ones_like(ref_bf), torch.frexp(ref_bf.abs().clamp_min(1e-30))[1] - 8)
    diff = (dx.double() - ref_bf).abs()
    print(f"K={K} C={C} M={M}: max |dx - ref| / ulp = {(diff / ulp).max().item():.3f}")
    assert (diff <= ulp).all()
    _check_partials(part, dx, z, C)


def test_head_dgrad_bn_fp32_activations():
    K, C, M = 3, 64, 257
    be = NativeBackend(DEV, torch.float32)
    dl, w, z, sc, sh = _inputs(K, C, M, torch.float32)
    dx, part = _run(be, K, C, M, dl, w, z, sc, sh)
    keep, _, ref = _reference(K, dl, w, z, sc, sh)
    assert (dx[~keep] == 0).all()
    rel = ((dx.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"fp32 activations: max rel {rel:.3e}")
    assert rel < 1e-6
    _check_partials(part, dx, z, C)


def test_unet_multiclass_backward_runs_head_dgrad_kernel(monkeypatch):
    from deeplearning_mpi_amd.models import UNet, engine
    from deeplearning_mpi_amd.ops import cross_entropy

    monkeypatch.setattr(engine, "_HEAD_DGRAD", True)
    torch.manual_seed(0)
    m = UNet(out_classes=3).to(DEV)
    x = torch.randn(2, 3, 64, 64, device=DEV)
    y = torch.randint(3, (2, 64, 64), device=DEV)
    m.engine_setup(DEV)
    C = m._be.C
    cross_entropy(m(x), y).backward()
    torch.cuda.synchronize()
    assert C.head_dgrad_last() == 1
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    monkeypatch.setattr(engine, "_HEAD_DGRAD", False)   # the GEMM path stays reachable
    m.arena.zero_grad()
    cross_entropy(m(x), y).backward()
    torch.cuda.synchronize()
    assert C.head_dgrad_last() == 0
