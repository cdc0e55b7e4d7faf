"""tests/conv_ref.py (the fp64 reference the convolution kernels are tested against) against torch
autograd in fp64: F.conv2d, its gradients, and F.relu of an affine for the mask forms."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

F64 = torch.float64
REL = 1e-10

# (R, S, stride, pad) x odd H x W (and one even, one with W < R + pad reach)
GEOS = [R.Geo(1, 1, 1, 0), R.Geo(1, 1, 2, 0), R.Geo(3, 3, 1, 1), R.Geo(3, 3, 2, 1), R.Geo(3, 3, 1, 0),
        R.Geo(7, 7, 2, 3), R.Geo(7, 7, 1, 3)]
GRIDS = [(9, 11), (7, 7), (13, 14), (15, 16)]
CASES = [(g, hw) for g in GEOS for hw in GRIDS]


def _close(a, b):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= REL * max(1.0, b.abs().max().item())


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _setup(g, hw, N=2, C=5, K=6, seed=0):
    gen = torch.Generator().manual_seed(seed + 17 * g.R + g.stride + hw[0])
    H, W = hw
    P, Q = R.out_hw(H, W, g)
    x = torch.randn(N, H, W, C, generator=gen, dtype=F64)
    w = torch.randn(K, g.R, g.S, C, generator=gen, dtype=F64)
    dy = torch.randn(N, P, Q, K, generator=gen, dtype=F64)
    return gen, x, w, dy


@pytest.mark.parametrize("g,hw", CASES, ids=[f"{g.R}x{g.S}s{g.stride}p{g.pad}-{h}x{w}" for g, (h, w) in CASES])
def test_forward_and_gradients(g, hw):
    gen, x, w, dy = _setup(g, hw)
    K = w.shape[0]
    bias = torch.randn(K, generator=gen, dtype=F64)
    scale, shift = torch.randn(K, generator=gen, dtype=F64), torch.randn(K, generator=gen, dtype=F64)
    res = torch.randn(dy.shape, generator=gen, dtype=F64)
    xt, wt = _nchw(x).clone().requires_grad_(True), w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    conv = F.conv2d(xt, wt, bias, stride=g.stride, padding=g.pad)
    # forward: plain, and the full epilogue
    v, mag, pre = R.fwd(x, w, g, bias=bias)
    _close(_nchw(v), conv.detach())
    assert torch.equal(v, pre)
    _close(_nchw(mag), F.conv2d(_nchw(x).abs(), w.permute(0, 3, 1, 2).abs(), bias.abs(), stride=g.stride,
                                padding=g.pad))
    v, mag, pre = R.fwd(x, w, g, bias=bias, scale=scale, shift=shift, res=res, relu=True)
    _close(_nchw(v), F.relu(conv.detach() * scale[None, :, None, None] + shift[None, :, None, None] + _nchw(res)))
    _close(_nchw(pre), conv.detach())
    assert bool((mag >= v.abs() - 1e-12).all())
    (s1, s2), (a1, a2) = R.stats(pre)
    _close(s1, conv.detach().sum((0, 2, 3)))
    _close(s2, (conv.detach() ** 2).sum((0, 2, 3)))
    _close(a1, conv.detach().abs().sum((0, 2, 3)))
    # gradients
    conv.backward(_nchw(dy))
    wT = w.permute(3, 1, 2, 0).contiguous()    # [C, R, S, K]
    dx, dmag = R.dgrad(dy, wT, g, *hw)
    _close(_nchw(dx), xt.grad)
    assert bool((dmag >= dx.abs() - 1e-12).all())
    dres, dbias = torch.randn(x.shape, generator=gen, dtype=F64), torch.randn(x.shape[-1], generator=gen, dtype=F64)
    dx2, dmag2 = R.dgrad(dy, wT, g, *hw, res=dres, bias=dbias)
    _close(dx2, dx + dres + dbias)
    _close(dmag2, dmag + dres.abs() + dbias.abs())
    (c1, c2), _ = R.colsum(dx)
    _close(c1, xt.grad.sum((0, 2, 3)))
    _close(c2, (xt.grad ** 2).sum((0, 2, 3)))
    gw, gmag = R.wgrad(dy, x, g)
    _close(gw.reshape(w.shape), wt.grad.permute(0, 2, 3, 1))
    assert bool((gmag >= gw.abs() - 1e-12).all())


def test_stride2_rows_no_output_touches_are_res_plus_bias_only():
    """1x1 stride 2: three of the four sub-pixel phases have no tap; 13 x 14 has unequal phases."""
    g = R.Geo(1, 1, 2, 0)
    gen, x, w, dy = _setup(g, (13, 14))
    wT = w.permute(3, 1, 2, 0).contiguous()
    res, bias = torch.randn(x.shape, generator=gen, dtype=F64), torch.randn(x.shape[-1], generator=gen, dtype=F64)
    dx, mag = R.dgrad(dy, wT, g, 13, 14)
    assert bool((dx[:, 1::2] == 0).all()) and bool((dx[:, :, 1::2] == 0).all())
    assert bool((mag[:, 1::2] == 0).all()) and bool((dx[:, ::2, ::2] != 0).all())
    dx, _ = R.dgrad(dy, wT, g, 13, 14, res=res, bias=bias)
    assert torch.equal(dx[:, 1::2], (res + bias)[:, 1::2]) and torch.equal(dx[:, :, 1::2], (res + bias)[:, :, 1::2])


@pytest.mark.parametrize("form", ["y", "bits", "z"])
@pytest.mark.parametrize("g,hw", [(R.Geo(1, 1, 1, 0), (7, 9)), (R.Geo(3, 3, 1, 1), (9, 11)), (R.Geo(3, 3, 2, 1), (15, 15))],
                         ids=["1x1", "3x3", "3x3s2"])
def test_fused_bn_backward_epilogue(g, hw, form):
    """dx = mask * dgrad is the gradient through y = relu(z * mscale + mshift) of the conv's input, and
    the partials are the sums BN's backward needs."""
    gen, x, w, dy = _setup(g, hw, C=8, K=6, seed=3)
    C = x.shape[-1]
    wT = w.permute(3, 1, 2, 0).contiguous()
    z = torch.randn(x.shape, generator=gen, dtype=F64)
    z2 = torch.randn(x.shape, generator=gen, dtype=F64)
    msc, msh = torch.randn(C, generator=gen, dtype=F64), torch.randn(C, generator=gen, dtype=F64)
    zt = z.clone().requires_grad_(True)
    y = F.relu(zt * msc + msh)
    out = F.conv2d(_nchw(y), w.permute(0, 3, 1, 2), stride=g.stride, padding=g.pad)
    out.backward(_nchw(dy))
    want = zt.grad / msc          # d/dy, masked: zt.grad = mask * dgrad * msc
    if form == "y":
        mask = R.relu_mask(y=y.detach())
    elif form == "bits":
        pos = (y.detach() > 0).reshape(*y.shape[:-1], C // 8, 8).to(torch.int32)
        bits = (pos * 2 ** torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)
        mask = R.relu_mask(bits=bits)
    else:
        mask, pre, pmag = R.relu_mask(z=z, mscale=msc, mshift=msh)
        _close(pre, (z * msc + msh))
        _close(pmag, (z * msc).abs() + msh.abs())
    assert torch.equal(mask, y.detach() > 0)
    gv, gm = R.dgrad(dy, wT, g, *hw)
    dx, mag, parts = R.bnbwd_epilogue(gv, gm, mask, z, z2)
    _close(dx, want)
    assert bool((mag[~mask] == 0).all()) and torch.equal(mag[mask], gm[mask])
    f = dx.reshape(-1, C)
    for (s, a), ref in zip(parts, (f, f * z.reshape(-1, C), f * z2.reshape(-1, C))):
        _close(s, ref.sum(0))
        _close(a, ref.abs().sum(0))
    assert len(R.bnbwd_partials(dx, z)) == 2 and len(R.bnbwd_partials(dx)) == 1


def test_tolerance_helpers_are_the_bn_reference_ones():
    import bn_ref

    assert R.U is bn_ref.U and R.half_ulp_bf16 is bn_ref.half_ulp_bf16 and R.store_tol is bn_ref.store_tol
