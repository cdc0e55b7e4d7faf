"""The fp64 reference of tests/pool_ref.py against independent derivations on the CPU: torch's max_pool2d
(values, indices, autograd), interpolate(bilinear, align_corners=True) and its autograd,
adaptive_avg_pool2d, permute + pad, a direct triple loop for the space-to-depth layout and autograd for
the head gradient, all in fp64 at 1e-12 relative.  The GPU tests hold the HIP kernels to pool_ref; this
file holds pool_ref to torch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R

F64 = torch.float64
TOL = 1e-12

# every (k, s, p) x (N, H, W, C) of the GPU file's max-pool table
POOL_CASES = [(3, 2, 1, 2, 7, 9, 8), (3, 2, 1, 1, 1, 1, 8), (3, 2, 1, 1, 2, 3, 24), (3, 2, 1, 2, 16, 16, 64),
              (2, 2, 0, 2, 8, 6, 8), (2, 2, 0, 1, 7, 5, 40), (2, 2, 0, 2, 16, 24, 128), (2, 2, 0, 2, 8, 6, 24),
              (3, 1, 1, 1, 5, 6, 16), (2, 1, 0, 2, 4, 5, 8), (3, 3, 0, 1, 9, 7, 8), (5, 2, 2, 1, 9, 11, 8),
              (3, 2, 0, 1, 8, 8, 16), (4, 2, 1, 1, 10, 6, 8)]
UP_SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (16, 16), (33, 17), (257, 2), (2, 300)]


def _close(a, b):
    scale = b.abs().max().item()
    return (a - b).abs().max().item() <= TOL * max(scale, 1e-300)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _flat_index(idx, k, s, p, W):
    """pool_ref's window position -> torch's index into the H*W plane."""
    _, OH, OW, _ = idx.shape
    i = idx.long()
    ih = (torch.arange(OH) * s - p)[None, :, None, None] + i // k
    iw = (torch.arange(OW) * s - p)[None, None, :, None] + i % k
    return ih * W + iw


@pytest.mark.parametrize("fill", ["randn", "ties"])
@pytest.mark.parametrize("k,s,p,N,H,W,C", POOL_CASES)
def test_maxpool_matches_torch(k, s, p, N, H, W, C, fill):
    g = torch.Generator().manual_seed(k * 100 + s * 10 + p + H)
    if fill == "randn":
        x = torch.randn(N, H, W, C, generator=g, dtype=F64)
    else:   # integer values from a handful: almost every window ties
        x = torch.randint(-2, 2, (N, H, W, C), generator=g).to(F64)
    y, idx = R.maxpool(x, k, s, p)
    xt = _nchw(x).requires_grad_()
    yt, it = F.max_pool2d(xt, k, s, p, return_indices=True)
    assert torch.equal(y, _nhwc(yt.detach()))
    assert torch.equal(_flat_index(idx, k, s, p, W), _nhwc(it))
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    yt.backward(_nchw(dy))
    assert _close(R.maxpool_bwd(dy, idx, H, W, k, s, p), _nhwc(xt.grad))
    add = torch.randn(N, H, W, C, generator=g, dtype=F64)
    dx, mag = R.maxpool_bwd_terms(dy, idx, H, W, k, s, p, add)
    assert _close(dx, _nhwc(xt.grad) + add)
    assert bool((mag >= dx.abs() - 1e-12).all())


def test_maxpool_padding_nan_and_inf_windows():
    x = -1.0 - torch.rand(1, 4, 4, 8, dtype=F64)
    y, idx = R.maxpool(x, 3, 2, 1)
    assert bool((y < 0).all())                       # padding never wins
    assert int(idx[0, 0, 0, 0]) >= 4 and int(idx[0, 0, 0, 0]) % 3 >= 1   # an in-image tap of the corner window
    # a NaN wins over any number, and the first NaN stays
    x = torch.randn(1, 5, 5, 8, dtype=F64)
    x[0, 2, 1, 3] = float("nan")
    x[0, 2, 2, 3] = float("nan")
    y, idx = R.maxpool(x, 3, 1, 0)
    assert bool(y[0, 0, 0, 3].isnan()) and int(idx[0, 0, 0, 3]) == 2 * 3 + 1
    assert bool(y[0, 0, 1, 3].isnan()) and int(idx[0, 0, 1, 3]) == 2 * 3 + 0
    assert not bool(y[..., :3].isnan().any())
    # a window with nothing above -inf reports its first in-image tap, as torch does
    x = torch.randn(1, 5, 5, 8, dtype=F64)
    x[0, :2, :2, :] = float("-inf")
    y, idx = R.maxpool(x, 3, 2, 1)
    yt, it = F.max_pool2d(_nchw(x), 3, 2, 1, return_indices=True)
    assert torch.equal(y, _nhwc(yt)) and torch.equal(_flat_index(idx, 3, 2, 1, 5), _nhwc(it))
    assert float(y[0, 0, 0, 0]) == float("-inf") and int(idx[0, 0, 0, 0]) == 1 * 3 + 1


@pytest.mark.parametrize("H,W", UP_SIZES)
def test_bilinear_matches_torch(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(2, H, W, 3, generator=g, dtype=F64)
    gy = torch.randn(2, 2 * H, 2 * W, 3, generator=g, dtype=F64)
    xt = _nchw(x).requires_grad_()
    yt = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=True)
    yt.backward(_nchw(gy))
    assert _close(R.upsample(x), _nhwc(yt.detach()))
    assert _close(R.upsample_bwd(gy), _nhwc(xt.grad))
    # the terms of the bounds: weights are non-negative and sum to one; the footprint holds every weight
    mag, foot = R.upsample_terms(x)
    assert bool((mag >= R.upsample(x).abs() - 1e-12).all()) and bool((foot >= mag - 1e-12).all())
    A = R.bilinear2x_matrix(H)
    assert _close(A.sum(1), torch.ones(2 * H, dtype=F64)) and bool((A >= 0).all())
    assert bool(((A > 0) <= (R.bilinear2x_footprint(H) > 0)).all())


def test_bilinear_adjoint():
    """<A x, g> == <x, A^T g>."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 33, 17, 4, generator=g, dtype=F64)
    gy = torch.randn(2, 66, 34, 4, generator=g, dtype=F64)
    a, b = (R.upsample(x) * gy).sum().item(), (x * R.upsample_bwd(gy)).sum().item()
    assert abs(a - b) <= TOL * max(abs(a), abs(b))
    assert torch.equal(R.bilinear2x_matrix(1), torch.ones(2, 1, dtype=F64))


def test_float_coordinate_floor_equals_exact_floor():
    """The kernels compute o * fl((n-1)/(2n-1)) in fp32.  For every n <= 300 its floor is the exact
    coordinate's floor at every output index and it lies within 2u (n-1) of it: the footprint of the
    bounds (pool_ref.bilinear2x_footprint) is the one the kernels read."""
    for n in range(2, 301):
        o = np.arange(2 * n)
        s = np.float32(n - 1) / np.float32(2 * n - 1)
        f = o.astype(np.float32) * s
        assert f.dtype == np.float32
        exact = o * (n - 1) // (2 * n - 1)
        assert np.array_equal(np.floor(f).astype(np.int64), exact), n
        assert np.all(np.abs(f.astype(np.float64) - o * (n - 1) / (2 * n - 1)) <= 2 * R.U * (n - 1)), n
        # the backward's candidate rows: every output row that reads input h lies in the fp32 range
        # [floor((h - 1) / s), (h + 1) / s] even before the kernel widens it by one row each side
        i0 = exact
        i1 = np.minimum(i0 + 1, n - 1)
        h = np.arange(n)
        lo = np.floor((h - 1).astype(np.float32) / s).astype(np.int64)
        hi = ((h + 1).astype(np.float32) / s).astype(np.int64)
        for hh in range(n):
            rows = o[(i0 == hh) | (i1 == hh)]
            assert lo[hh] <= rows.min() and rows.max() <= hi[hh], (n, hh)


@pytest.mark.parametrize("HW", [1, 2, 49])
def test_avgpool_matches_torch(HW):
    g = torch.Generator().manual_seed(HW)
    x = torch.randn(3, HW, 24, generator=g, dtype=F64)
    xt = x.permute(0, 2, 1).reshape(3, 24, HW, 1).clone().requires_grad_()
    yt = F.adaptive_avg_pool2d(xt, 1)
    dy = torch.randn(3, 24, generator=g, dtype=F64)
    yt.backward(dy[:, :, None, None])
    assert _close(R.avgpool(x), yt.detach().reshape(3, 24))
    assert _close(R.avgpool_bwd(dy, HW), xt.grad.reshape(3, 24, HW).permute(0, 2, 1))


def test_layouts_match_permute_and_pad():
    g = torch.Generator().manual_seed(11)
    for C, Cpad in [(1, 8), (3, 8), (4, 8), (8, 8), (9, 16)]:
        x = torch.randn(2, C, 5, 7, generator=g, dtype=F64)
        assert torch.equal(R.nchw_to_nhwc_pad(x, Cpad), F.pad(x.permute(0, 2, 3, 1), (0, Cpad - C)))
    x = torch.randn(257, 5, generator=g, dtype=F64)
    assert torch.equal(R.pad_cast(x, 8), F.pad(x, (0, 3)))
    assert torch.equal(R.pad_cast(x.float(), 16, torch.bfloat16), F.pad(x.float().to(torch.bfloat16), (0, 11)))


@pytest.mark.parametrize("H,W,pad", [(5, 7, 3), (8, 8, 1)])
def test_s2d_matches_triple_loop(H, W, pad):
    g = torch.Generator().manual_seed(H)
    N, C, CS = 2, 3, 4
    U_, V = (H + 2 * pad + 1) // 2, (W + 2 * pad + 1) // 2
    x = torch.randn(N, C, H, W, generator=g, dtype=F64)
    want = torch.zeros(N, U_, V, 4 * CS, dtype=F64)
    for u in range(U_):
        for v in range(V):
            for j in range(4 * CS):
                slot, c = divmod(j, CS)
                h, w = 2 * u + slot // 2 - pad, 2 * v + slot % 2 - pad
                if c < C and 0 <= h < H and 0 <= w < W:
                    want[:, u, v, j] = x[:, c, h, w]
    assert torch.equal(R.s2d(x, pad, U_, V, CS), want)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_head_dgrad_matches_autograd(K):
    g = torch.Generator().manual_seed(K)
    M, C = 37, 24
    z = torch.randn(M, C, generator=g, dtype=F64)
    scale, shift = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.randn(C, generator=g, dtype=F64)
    w, dl = torch.randn(C, K, generator=g, dtype=F64), torch.randn(M, K, generator=g, dtype=F64)
    zt = z.clone().requires_grad_()
    a = torch.relu(zt * scale + shift)
    a.retain_grad()
    (a @ w).backward(dl)                               # logits [M, K] = a w
    dx, sums, mags = R.head_dgrad(dl, w, z, scale, shift)
    assert _close(dx, a.grad * (a.detach() > 0))       # the gradient of the ReLU output, masked
    assert _close(dx * scale, zt.grad)
    assert _close(sums[0], dx.sum(0)) and _close(sums[1], (dx * z).sum(0))
    assert bool((mags >= sums.abs() - 1e-12).all())
    dxt, mag = R.head_dgrad_terms(dl, w, z, scale, shift)
    assert torch.equal(dxt, dx) and bool((mag >= dx.abs() - 1e-12).all())
    assert torch.equal(R.relu_mask(z, scale, shift), a.detach() > 0)


def test_apply_relu_rounds_to_the_storage_type():
    z = torch.tensor([[-1.0, 0.0, 0.125, 3.0]], dtype=F64)
    y = R.apply_relu(z, torch.tensor([2.0] * 4), torch.tensor([0.125] * 4), torch.bfloat16)
    assert torch.equal(y, torch.tensor([[0.0, 0.125, 0.375, 6.125]], dtype=F64))
    y = R.apply_relu(torch.tensor([[1.0 + 2.0 ** -10]]), torch.ones(1), torch.zeros(1), torch.bfloat16)
    assert y.item() == 1.0
