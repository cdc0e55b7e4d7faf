"""fp64 reference of the training BatchNorm family, stage by stage, as the kernels define the
operation (the header of csrc/kernels/bn.hip) -- explicit formulas in plain torch, written from the
definition of batch normalisation and its derivative, not from the kernels' code.

Every function takes tensors of any floating type (and device), converts to fp64 and returns fp64
(mask bits: uint8).  Activations are 2-D ``[M, C]`` (rows = N*H*W pixels); ``view`` cuts the
channel slice of an :class:`Act` out of its wider buffer.  tests/test_bn_ref_cpu.py ties the
composition of these stages to torch autograd in fp64.
"""
import torch

from deeplearning_mpi_amd.ops.act import Act

F64 = torch.float64


def d(t):
    return None if t is None else t.to(F64)


def view(a: Act) -> torch.Tensor:
    """The [M, C] channel slice of an Act (a view of its buffer)."""
    return a.buf[:, a.off:a.off + a.C]


# ------------------------------------------------------------------ forward
def sums(x):
    """Per-channel sum x and sum x^2."""
    x = d(x)
    return x.sum(0), (x * x).sum(0)


def fwd_finalize(s1, s2, count, gamma=None, beta=None, eps=1e-5, running_mean=None, running_var=None, momentum=0.1):
    """mean, biased variance clamped at 0, invstd, scale, shift; the running statistics (when given)
    move by ``momentum`` towards the batch mean and torch's unbiased batch variance."""
    s1, s2 = d(s1), d(s2)
    count = float(count)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = invstd if gamma is None else d(gamma) * invstd
    shift = -mean * scale if beta is None else d(beta) - mean * scale
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift)
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1.0 else var
        out["unbiased"] = unbiased
        out["running_mean"] = (1.0 - momentum) * d(running_mean) + momentum * mean
        out["running_var"] = (1.0 - momentum) * d(running_var) + momentum * unbiased
    return out


def apply_terms(x, scale, shift, res=None, rscale=None, rshift=None):
    """(pre-activation, sum of the absolute values of its terms)."""
    a = d(x) * d(scale)
    pre = a + d(shift)
    mag = a.abs() + d(shift).abs().expand_as(a)
    if res is not None:
        r = d(res)
        if rscale is not None:
            r = r * d(rscale)
            pre = pre + (r + d(rshift))
            mag = mag + r.abs() + d(rshift).abs()
        else:
            pre = pre + r
            mag = mag + r.abs()
    return pre, mag


def apply(x, scale, shift, res=None, rscale=None, rshift=None, relu=True):
    """relu(x*scale + shift [+ res | + res*rscale + rshift])."""
    pre, _ = apply_terms(x, scale, shift, res, rscale, rshift)
    return pre.clamp_min(0.0) if relu else pre


def mask_bits(y_stored):
    """[M, C/8] bytes: bit e of byte (row, g) set when the stored y[row][8g + e] > 0."""
    M, C = y_stored.shape
    pos = (y_stored > 0).reshape(M, C // 8, 8).to(torch.int32)
    w = (2 ** torch.arange(8, device=y_stored.device, dtype=torch.int32))
    return (pos * w).sum(-1).to(torch.uint8)


# ------------------------------------------------------------------ backward
def masked(dy, ymask=None):
    """dyr = dy * [stored ymask > 0] (dy itself without a mask)."""
    dy = d(dy)
    return dy if ymask is None else torch.where(ymask > 0, dy, torch.zeros_like(dy))


def bwd_reduce(dy, ymask, x, mean, invstd):
    """s1 = sum dyr, s2 = sum dyr * xhat with xhat = (x - mean) * invstd."""
    dyr = masked(dy, ymask)
    xhat = (d(x) - d(mean)) * d(invstd)
    return dyr.sum(0), (dyr * xhat).sum(0)


def bwd_reduce_raw(dy, ymask, z, mean, invstd):
    """The raw_z form: s2 = invstd * (sum dyr*z - mean * s1)."""
    dyr = masked(dy, ymask)
    s1 = dyr.sum(0)
    sz = (dyr * d(z)).sum(0)
    return s1, raw_to_xhat(s1, sz, mean, invstd), sz


def raw_to_xhat(s1, sz, mean, invstd):
    return d(invstd) * (d(sz) - d(mean) * d(s1))


def bwd_finalize(s1, s2, count, gamma, mean, invstd, dgamma0=None, dbeta0=None):
    """dbeta += s1, dgamma += s2 and the coefficients of dx = k1*dyr + k2*x + k3:
    dx = gamma*invstd * (dyr - s1/count - xhat * s2/count), expanded in x."""
    s1, s2, mean, invstd = d(s1), d(s2), d(mean), d(invstd)
    count = float(count)
    g = torch.ones_like(invstd) if gamma is None else d(gamma)
    k1 = g * invstd
    k2 = -k1 * invstd * s2 / count
    k3 = -k1 * s1 / count - k2 * mean
    out = dict(k1=k1, k2=k2, k3=k3)
    if dgamma0 is not None:
        out["dgamma"] = d(dgamma0) + s2
    if dbeta0 is not None:
        out["dbeta"] = d(dbeta0) + s1
    return out


def bwd_apply_terms(dyr, x, k1, k2, k3):
    a, b = d(k1) * d(dyr), d(k2) * d(x)
    return a + b + d(k3), a.abs() + b.abs() + d(k3).abs()


def bwd_apply(dyr, x, k1, k2, k3):
    return bwd_apply_terms(dyr, x, k1, k2, k3)[0]


def dual_weights(W, k1, k2, k3):
    """w2 [C][2K] = {W*k1, W*k2}, b [C] = sum_k W*k3 and sum_k |W*k3|."""
    W = d(W)
    t = W * d(k3)
    return torch.cat([W * d(k1), W * d(k2)], 1), t.sum(1), t.abs().sum(1)


# ------------------------------------------------------------------ tolerances
U = 2.0 ** -24   # unit roundoff of fp32 (round to nearest)


def half_ulp_bf16(ref):
    """Half a bf16 ulp of ref: 2^(floor(log2|ref|) - 8); 0 at ref == 0."""
    m, e = torch.frexp(ref.abs())   # |ref| = m * 2^e, m in [0.5, 1): floor(log2|ref|) = e - 1
    h = torch.ldexp(torch.ones_like(ref), e - 9)
    return torch.where(ref == 0, torch.zeros_like(ref), h)


def store_tol(ref, dtype):
    """The storage rounding of an activation: half a bf16 ulp, nothing for fp32."""
    return half_ulp_bf16(ref) if dtype == torch.bfloat16 else torch.zeros_like(ref)
