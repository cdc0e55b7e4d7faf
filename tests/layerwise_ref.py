"""Shared by tests/test_layerwise_optim_{cpu,gpu}.py: the parameter set on which segment mapping,
tails and chunk edges can break, and an independent per-tensor fp64 LARS / LAMB (written from the
definitions in the README, not from the kernels)."""
import math

import torch
import torch.nn as nn

C = 4096   # chunk size of the layer-wise kernels
NUMELS = [1, 3, 4, 5, 15, 16, 17, C - 1, C, C + 1, 2 * C + 1, 3 * C + 3]
QUIET_STEP = 1   # the step (0-based) on which `quiet` gets a zero gradient


class Bag(nn.Module):
    """2-D tensors of the edge-case sizes (adapted), a 7x7 conv weight (stored permuted by the
    arena), two 1-D tensors (excluded by default), an all-zero weight and `quiet`."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.mats = nn.ParameterList([nn.Parameter(torch.randn(1, n, generator=g)) for n in NUMELS])
        self.conv = nn.Conv2d(3, 64, 7, bias=False)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(64, 3, 7, 7, generator=g) * 0.1)
        self.v10 = nn.Parameter(torch.randn(10, generator=g))
        self.v1000 = nn.Parameter(torch.randn(1000, generator=g))
        self.zero = nn.Parameter(torch.zeros(8, 33))
        self.quiet = nn.Parameter(torch.randn(5, 77, generator=g))


def make_grads(model, steps, seed=11, nan_step=None):
    """Per step, one CPU fp32 gradient per parameter (in model.parameters() order)."""
    g = torch.Generator().manual_seed(seed)
    names = [n for n, _ in model.named_parameters()]
    out = []
    for s in range(steps):
        gs = [torch.randn(p.shape, generator=g) * 0.3 for p in model.parameters()]
        if s == QUIET_STEP:
            gs[names.index("quiet")].zero_()
        out.append(gs)
    if nan_step is not None:
        bad = [x.clone() for x in out[nan_step]]
        bad[names.index("mats.9")].view(-1)[5] = float("nan")
        out.insert(nan_step, bad)
    return out


def lr_at(base, s, sched):
    """The README's schedule: s = updates applied so far."""
    sched = sched or {}
    kind, W, T = sched.get("kind", "constant"), sched.get("warmup_steps", 0), sched.get("total_steps", 0)
    lo, power = sched.get("min_lr", 0.0), sched.get("power", 2.0)
    if s < W:
        return base * (s + 1) / W
    q = min(1.0, (s - W) / max(1, T - W))
    if kind == "cosine":
        return lo + (base - lo) * 0.5 * (1 + math.cos(math.pi * q))
    if kind == "poly":
        return lo + (base - lo) * (1 - q) ** power
    return base


def ref_lars(ws, grads, excluded, lr, momentum=0.9, wd=0.0, nesterov=False, tc=1e-3, eps=1e-9, sched=None):
    """ws: fp64 tensors; grads[step][i]; excluded[i] -> no decay, ratio 1.  Returns (ws, ms, ratios of
    the last step, lr of the last step)."""
    ws = [w.double().clone() for w in ws]
    ms = [torch.zeros_like(w) for w in ws]
    ratios, lr_t = [], None
    for s, gs in enumerate(grads):
        lr_t = lr_at(lr, s, sched)
        ratios = []
        for i, (w, g) in enumerate(zip(ws, gs)):
            g = g.double()
            wdi = 0.0 if excluded[i] else wd
            wn, gn = float(w.norm()), float(g.norm())
            r = 1.0
            if not excluded[i] and wn > 0 and gn > 0:
                r = tc * wn / (gn + wdi * wn + eps)
            d = r * (g + wdi * w)
            ms[i] = d.clone() if s == 0 else momentum * ms[i] + d
            w -= lr_t * (d + momentum * ms[i] if nesterov else ms[i])
            ratios.append(r)
    return ws, ms, torch.tensor(ratios, dtype=torch.float64), lr_t


def ref_lamb(ws, grads, excluded, lr, betas=(0.9, 0.999), eps=1e-6, wd=0.01, sched=None):
    ws = [w.double().clone() for w in ws]
    ms = [torch.zeros_like(w) for w in ws]
    vs = [torch.zeros_like(w) for w in ws]
    b1, b2 = betas
    ratios, lr_t = [], None
    for s, gs in enumerate(grads):
        lr_t = lr_at(lr, s, sched)
        t = s + 1
        ratios = []
        for i, (w, g) in enumerate(zip(ws, gs)):
            g = g.double()
            wdi = 0.0 if excluded[i] else wd
            ms[i] = b1 * ms[i] + (1 - b1) * g
            vs[i] = b2 * vs[i] + (1 - b2) * g * g
            u = (ms[i] / (1 - b1 ** t)) / ((vs[i] / (1 - b2 ** t)).sqrt() + eps) + wdi * w
            wn, un = float(w.norm()), float(u.norm())
            r = wn / un if (not excluded[i] and wn > 0 and un > 0) else 1.0
            w -= lr_t * r * u
            ratios.append(r)
    return ws, ms, vs, torch.tensor(ratios, dtype=torch.float64), lr_t


def rel_err(a, b):
    """max|a - b| / max|b| (the bound of tests/test_kernels_gpu.py); an all-zero b must be met exactly."""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(b.abs().max())
    err = float((a - b).abs().max())
    return err / den if den > 0 else (0.0 if err == 0 else float("inf"))


def set_grads(model, gs, device):
    for p, g in zip(model.parameters(), gs):
        if p.grad is None:
            p.grad = g.to(device).clone()
        else:
            p.grad.copy_(g.to(device))


def arena_state(arena, flat_state):
    """Per-parameter views (logical shape) of a flat state array laid out like arena.flat."""
    return [flat_state.as_strided(tuple(p.shape), arena._strides(tuple(p.shape), arena.layouts[i]), arena.offsets[i])
            for i, p in enumerate(arena.params)]


def padding_mask(arena):
    m = torch.ones(arena.total, dtype=torch.bool)
    for i, p in enumerate(arena.params):
        m[arena.offsets[i]:arena.offsets[i] + p.numel()] = False
    return m
