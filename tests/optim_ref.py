"""fp64 reference of the parameter-side kernels (csrc/kernels/optim.hip, cast.hip, util.hip): SGD, Adam /
AdamW, the gradient norm and its clip coefficient, the zero-padded weight re-layout with its bf16
rounding, and the indexed gather -- explicit formulas in plain torch, written from the definitions of
the operations (torch.optim, clip_grad_norm_), not from the kernels' code, and without RefBackend.

Every function takes tensors of any floating type (and device), works in fp64 and changes none of its
arguments.  The scalar hyper-parameters are used as given: the kernels receive lr, momentum, dampening,
wd, eps and the betas of the moment updates rounded to fp32, so a caller that compares with a kernel
passes ``f32(value)``.  Adam's bias corrections are torch's: ``1 - beta**t`` of the DOUBLE betas
(``bc_betas``), whatever the moment updates use.  tests/test_optim_ref_cpu.py ties these formulas to
torch.optim.SGD / Adam / AdamW, clip_grad_norm_, RefBackend.cast_weights and Tensor.to(bfloat16).
"""
import math
import struct

import torch

from bn_ref import F64, U   # noqa: F401  (re-exported: one vocabulary of bounds)


def f32(x):
    """The fp32 rounding of a host scalar, as a Python float (what ``(float)x`` of the binding keeps)."""
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def skipped(skip):
    """The kernels' rule: any non-zero skip value skips, and NaN is non-zero; None, 0.0 and -0.0 run."""
    if skip is None:
        return False
    s = float(skip.reshape(-1)[0]) if torch.is_tensor(skip) else float(skip)
    return s != 0.0   # NaN != 0.0 is True


# ------------------------------------------------------------------ SGD
def sgd(p, g, m, lr, momentum, dampening, wd, nesterov, first, skip=None, detail=False):
    """-> (p, m) after one update (fp64):
        d = g + wd p;  m = d if first else momentum m + (1 - dampening) d;  d = d + momentum m (nesterov) or m;
        p = p - lr d.
    momentum == 0 leaves m as it was (and d = g + wd p); nesterov is not coupled to dampening.  A skipped
    call returns p and m unchanged.  detail=True adds the dict of the sums of the absolute terms of m, d and p."""
    p, g = p.to(F64), g.to(F64)
    m = None if m is None else m.to(F64)
    if skipped(skip):
        return (p, m, None) if detail else (p, m)
    d = g + wd * p
    Md = g.abs() + (wd * p).abs()
    Mm = None
    if momentum != 0:
        if first:
            m, Mm = d, Md
        else:
            Mm = (momentum * m).abs() + abs(1 - dampening) * Md
            m = momentum * m + (1 - dampening) * d
        if nesterov:
            Md = Md + abs(momentum) * Mm
            d = d + momentum * m
        else:
            d, Md = m, Mm
    Mp = p.abs() + abs(lr) * Md
    p = p - lr * d
    return (p, m, {"Mm": Mm, "Md": Md, "Mp": Mp}) if detail else (p, m)


# ------------------------------------------------------------------ Adam / AdamW
def adam(p, g, m, v, lr, b1, b2, eps, wd, adamw, t, coef=1.0, skip=None, writeback=False, bc_betas=None,
         detail=False):
    """-> (p, g, m, v) after update number ``t`` (fp64):
        g' = g coef;  adamw: p = p (1 - lr wd), else g' = g' + wd p;
        m = m + (g' - m)(1 - b1)   (torch's lerp);  v = b2 v + (1 - b2) g'^2;
        p = p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),   bc = 1 - beta^t of ``bc_betas`` (default (b1, b2)).
    The returned g is g coef when ``writeback`` and coef != 1 (the clipped gradients stay visible), else g.
    A skipped call returns everything unchanged.  detail=True adds the intermediates the bounds need."""
    p, g, m, v = p.to(F64), g.to(F64), m.to(F64), v.to(F64)
    if skipped(skip):
        return (p, g, m, v, None) if detail else (p, g, m, v)
    coef = float(coef)
    B1, B2 = (b1, b2) if bc_betas is None else bc_betas
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    ge = g * coef
    Mg = ge.abs()
    gout = ge if (writeback and coef != 1.0) else g
    p1 = p
    if wd != 0:
        if adamw:
            p1 = p * (1 - lr * wd)
        else:
            Mg = Mg + (wd * p).abs()
            ge = ge + wd * p
    Mm = m.abs() + abs(1 - b1) * (Mg + m.abs())
    m = m + (ge - m) * (1 - b1)
    Mv = (v * b2).abs() + abs(1 - b2) * Mg * Mg
    v = v * b2 + (1 - b2) * ge * ge
    sq = v.sqrt()
    den = sq / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m / den
    out = (p1 - upd, gout, m, v)
    if detail:
        return out + ({"Mg": Mg, "Mm": Mm, "Mv": Mv, "p1": p1, "sq": sq, "den": den, "upd": upd, "bc1": bc1,
                       "bc2": bc2},)
    return out


# ------------------------------------------------------------------ gradient norm and clip coefficient
def grad_norm(g, max_norm):
    """-> (norm, coef, nonfinite): the L2 norm of g (fp64), clip_grad_norm_'s scale
    min(1, max_norm / (norm + 1e-6)) and a flag for a NaN or infinite norm.  NaN norm: coef 1 (no comparison
    with NaN holds, so nothing is scaled); infinite norm: coef 0."""
    norm = float(g.to(F64).pow(2).sum().sqrt())
    if math.isnan(norm):
        return norm, 1.0, 1.0
    if math.isinf(norm):
        return norm, 0.0, 1.0
    return norm, min(1.0, max_norm / (norm + 1e-6)), 0.0


# ------------------------------------------------------------------ weight re-layout and bf16 rounding
def relayout(src, dims, valid, strides):
    """The 4-D destination [dims] (a new fp32 tensor) of a cast_weights entry: element (i0..i3) is
    src.view(-1)[sum i_k strides_k] where every i_k < valid_k, and +0.0 elsewhere."""
    out = torch.zeros(tuple(dims), dtype=src.dtype, device=src.device)
    if min(valid) > 0:
        out[:valid[0], :valid[1], :valid[2], :valid[3]] = src.as_strided(tuple(valid), tuple(strides))
    return out


def bf16_bits(x):
    """Round-to-nearest-even of fp32 values to bf16 on the bit patterns -> the 16 bits as int32 in
    [0, 65535].  Add 0x7fff plus the lowest kept bit and drop the low half: a tie goes to the even
    neighbour, a carry runs into the exponent (the largest finite bf16 plus half an ulp becomes inf).
    A NaN keeps its sign and high payload and has its quiet bit set, so it cannot round to inf."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff
    nan = ((b & 0x7f800000) == 0x7f800000) & ((b & 0x007fffff) != 0)
    return torch.where(nan, (b >> 16) | 0x40, r).to(torch.int32)


def bf16_round(x):
    """fp32 values rounded to bf16 and widened again (fp32)."""
    return (bf16_bits(x) << 16).to(torch.int32).view(torch.float32).reshape(x.shape)


# ------------------------------------------------------------------ gather
def gather(dst, src, idx, accumulate=False):
    """-> the new dst (its own type): dst.view(-1)[i] (+)= src.view(-1)[idx[i]] for i < idx.numel(), a
    negative index reading as zero in both modes; the tail of dst stays.  Accumulation is in dst's type
    (one addition per element: exact to compare with)."""
    out = dst.clone().reshape(-1)
    sv = src.reshape(-1)
    val = torch.where(idx >= 0, sv[idx.clamp_min(0)], torch.zeros((), dtype=sv.dtype, device=sv.device))
    n = idx.numel()
    out[:n] = out[:n] + val if accumulate else val
    return out.reshape(dst.shape)
