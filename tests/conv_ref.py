"""fp64 reference of the convolution family -- forward with its epilogue, data gradient (the true
adjoint, stride 2 included) with the fused BN-backward epilogue, weight gradient -- written from the
definition of a convolution as explicit sums over taps in plain torch, not from the kernels' code.

Layouts are the kernels': activations NHWC ``[N, H, W, C]``, forward weights ``[K, R, S, C]``, data
gradient weights ``wT [C, R, S, K]``, weight gradients ``[Ko, R*S, C]``.  Inputs of any floating type
are widened to fp64, so a caller passes the exact bf16 / fp32 values a kernel read.  Every value comes
with ``mag``, the sum of the absolute values of the terms that form it: the rounding-count bounds of
tests/test_conv_family_fp64_gpu.py are multiples of ``U * mag``.  tests/test_conv_ref_cpu.py ties
these formulas to torch autograd in fp64.
"""
from collections import namedtuple

import torch

from bn_ref import F64, U, d, half_ulp_bf16, store_tol  # noqa: F401  (re-exported for the tests)

Geo = namedtuple("Geo", "R S stride pad")


def out_hw(H, W, g: Geo):
    return (H + 2 * g.pad - g.R) // g.stride + 1, (W + 2 * g.pad - g.S) // g.stride + 1


def _taps(g: Geo, H, W):
    """(r, s, the output rows p and columns q whose tap (r, s) lies inside the image)."""
    P, Q = out_hw(H, W, g)
    for r in range(g.R):
        p = [i for i in range(P) if 0 <= i * g.stride - g.pad + r < H]
        if not p:
            continue
        for s in range(g.S):
            q = [j for j in range(Q) if 0 <= j * g.stride - g.pad + s < W]
            if q:
                yield r, s, p[0], p[-1] + 1, q[0], q[-1] + 1


def _conv(x, w, g: Geo):
    """y[n, p, q, k] = sum_{r, s, c} x[n, p*stride - pad + r, q*stride - pad + s, c] * w[k, r, s, c]."""
    N, H, W, _ = x.shape
    P, Q = out_hw(H, W, g)
    y = torch.zeros(N, P, Q, w.shape[0], dtype=F64, device=x.device)
    for r, s, p0, p1, q0, q1 in _taps(g, H, W):
        h0, w0 = p0 * g.stride - g.pad + r, q0 * g.stride - g.pad + s
        xs = x[:, h0:h0 + (p1 - p0 - 1) * g.stride + 1:g.stride, w0:w0 + (q1 - q0 - 1) * g.stride + 1:g.stride]
        y[:, p0:p1, q0:q1] += xs @ w[:, r, s].t()
    return y


def fwd(x, w, g: Geo, bias=None, scale=None, shift=None, res=None, relu=False):
    """(value, mag) of relu?( (conv(x, w) + bias) * scale + shift + res ), and the un-activated conv +
    bias (the value BN statistics are taken of) as a third result."""
    x, w = d(x), d(w)
    v, mag = _conv(x, w, g), _conv(x.abs(), w.abs(), g)
    if bias is not None:
        v, mag = v + d(bias), mag + d(bias).abs()
    pre = v
    if scale is not None:
        v, mag = v * d(scale) + d(shift), mag * d(scale).abs() + d(shift).abs()
    if res is not None:
        v, mag = v + d(res), mag + d(res).abs()
    if relu:
        v = v.clamp_min(0.0)
    return v, mag, pre


def stats(y):
    """Per-channel (sum y, sum y^2) over the pixels and their (sum |y|, sum y^2)."""
    y = d(y).reshape(-1, y.shape[-1])
    return (y.sum(0), (y * y).sum(0)), (y.abs().sum(0), (y * y).sum(0))


def _adjoint(dy, wT, g: Geo, H, W):
    """dx[n, h, w, c] = sum over (p, q, r, s) with p*stride - pad + r == h, q*stride - pad + s == w of
    dy[n, p, q, :] . wT[c, r, s, :] -- scattered tap by tap, so an input pixel no output touches gets
    no term at all."""
    N = dy.shape[0]
    dx = torch.zeros(N, H, W, wT.shape[0], dtype=F64, device=dy.device)
    for r, s, p0, p1, q0, q1 in _taps(g, H, W):
        h0, w0 = p0 * g.stride - g.pad + r, q0 * g.stride - g.pad + s
        dx[:, h0:h0 + (p1 - p0 - 1) * g.stride + 1:g.stride, w0:w0 + (q1 - q0 - 1) * g.stride + 1:g.stride] += \
            dy[:, p0:p1, q0:q1] @ wT[:, r, s].t()
    return dx


def dgrad(dy, wT, g: Geo, H, W, res=None, bias=None):
    """(value, mag) of the data gradient + bias + res; dy [N, P, Q, K], wT [C, R, S, K]."""
    dy, wT = d(dy), d(wT)
    assert tuple(dy.shape[1:3]) == out_hw(H, W, g)
    v, mag = _adjoint(dy, wT, g, H, W), _adjoint(dy.abs(), wT.abs(), g, H, W)
    if bias is not None:
        v, mag = v + d(bias), mag + d(bias).abs()
    if res is not None:
        v, mag = v + d(res), mag + d(res).abs()
    return v, mag


def colsum(dx):
    """Per-channel {sum dx, sum dx^2} of a stored gradient, with their sums of absolute terms."""
    return stats(dx)


def relu_mask(y=None, bits=None, z=None, mscale=None, mshift=None):
    """The ReLU mask of the fused BN-backward epilogue, bool [..., C]: stored y > 0, the mask bits
    (bit e of byte g: channel 8g + e), or z * mscale + mshift > 0.  The last form also returns the
    fp64 pre-activation and the sum of its absolute terms (the caller excludes |pre| <= 2 U mag)."""
    if y is not None:
        return y > 0
    if bits is not None:
        w = 2 ** torch.arange(8, device=bits.device, dtype=torch.int32)
        return ((bits.to(torch.int32).unsqueeze(-1) & w) != 0).reshape(*bits.shape[:-1], bits.shape[-1] * 8)
    a = d(z) * d(mscale)
    pre = a + d(mshift)
    return pre > 0, pre, a.abs() + d(mshift).abs()


def bnbwd_epilogue(g_val, g_mag, mask, z=None, z2=None):
    """dx = mask * dgrad and the per-channel partials {sum dx, sum dx z [, sum dx z2]} of that fp64 dx
    (the kernels take theirs of the STORED dx: the tests recompute these from the stored tensor)."""
    dx = torch.where(mask, g_val, torch.zeros_like(g_val))
    mag = torch.where(mask, g_mag, torch.zeros_like(g_mag))
    return dx, mag, bnbwd_partials(dx, z, z2)


def bnbwd_partials(dx, z=None, z2=None):
    """[(sum, sum of absolute terms)] of dx, dx*z [, dx*z2] per channel."""
    dx = d(dx).reshape(-1, dx.shape[-1])
    out = [(dx.sum(0), dx.abs().sum(0))]
    for t in (z, z2):
        if t is not None:
            p = dx * d(t).reshape(-1, dx.shape[-1])
            out.append((p.sum(0), p.abs().sum(0)))
    return out


def wgrad(dy, x, g: Geo):
    """(value, mag) [Ko, R*S, C]: grad[k, r*S + s, c] = sum_{n, p, q} dy[n, p, q, k] *
    x[n, p*stride - pad + r, q*stride - pad + s, c]."""
    dy, x = d(dy), d(x)
    N, H, W, C = x.shape
    assert tuple(dy.shape[1:3]) == out_hw(H, W, g)
    Ko = dy.shape[-1]
    out = [torch.zeros(Ko, g.R * g.S, C, dtype=F64, device=x.device) for _ in range(2)]
    for r, s, p0, p1, q0, q1 in _taps(g, H, W):
        h0, w0 = p0 * g.stride - g.pad + r, q0 * g.stride - g.pad + s
        xs = x[:, h0:h0 + (p1 - p0 - 1) * g.stride + 1:g.stride, w0:w0 + (q1 - q0 - 1) * g.stride + 1:g.stride]
        a, b = dy[:, p0:p1, q0:q1].reshape(-1, Ko), xs.reshape(-1, C)
        out[0][:, r * g.S + s] = a.t() @ b
        out[1][:, r * g.S + s] = a.abs().t() @ b.abs()
    return out[0], out[1]
