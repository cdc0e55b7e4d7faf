"""Inputs and the plain fp64 reference of the OHEM tests (tests/test_ohem_cpu.py, test_ohem_gpu.py).

Inputs come from a seeded CPU generator, so the precondition of every comparison is checked without a GPU: the fp32
kernel and the fp64 reference select the same set only if no loss lies near the cut, hence `select` asserts -- it
never skips -- that the k-th and (k+1)-th largest losses differ by more than 1e-4 and, with a threshold, that no
valid loss lies within 1e-4 of tau (the fp32 per-pixel loss is good to about 1e-6).  SEEDS were chosen on the CPU
so that every case passes."""
import math

import torch
import torch.nn.functional as F

N, H, W = 2, 17, 23   # 782 pixels: partial blocks and tail lanes (the shape of tests/test_pixel_ce_gpu.py)
# (keep_ratio, min_kept, thresh): the ratio decides / min_kept decides / tau decides (t_k > tau) / the issue's
# (0.9, 0.999), where tau = 0.001 is below every loss of these random logits, so again tau / t_k decides under a
# threshold (tau = 1.2 > t_k)
SETTINGS = [(0.25, 1, None), (0.05, 100, None), (0.1, 1, 0.7), (0.9, 1, 0.999), (0.9, 1, 0.3)]
SEEDS = {2: 1, 3: 1, 4: 1, 5: 1, 21: 1, 40: 1, "hard": 1, "soft": 3, "wrap": 4}


def softmax_inputs(K, seed, shape=(N, H, W)):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, K, generator=g)   # class-last storage
    y = torch.randint(K, shape, generator=g)
    y[0, :3] = -100
    y[-1, 5, 7] = K + 3   # out of range: ignored as well
    w = torch.rand(K, generator=g) + 0.5
    return x, y, w


def binary_inputs(kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, generator=g) * 2
    t = torch.rand(N, H, W, generator=g)
    return x, (t > 0.5).float() if kind == "hard" else t


def select(l, valid, keep_ratio, min_kept, thresh):
    """fp64 losses l, validity mask (both flat) -> (selection mask, k), after the precondition's assertions."""
    lv = l[valid]
    nv = lv.numel()
    k = min(nv, max(min_kept, math.ceil(keep_ratio * nv)))
    cut = lv.kthvalue(nv - k + 1).values
    if k < nv:
        assert cut - lv.kthvalue(nv - k).values > 1e-4, "the k-th and (k+1)-th largest losses are too close"
    if thresh is not None:
        tau = torch.tensor(-math.log(thresh), dtype=torch.float32).double()
        assert (lv - tau).abs().min() > 1e-4, "a loss lies too close to tau"
        cut = torch.minimum(cut, tau)
    return valid & (l >= cut), k


def softmax_reference(x, y, w, keep_ratio, min_kept, thresh):
    """x fp32 [N, K, H, W] (any strides), y, w or None -> fp64 (loss, gradient, selection mask [N, H, W], k)."""
    K = x.shape[1]
    xr = x.detach().double().requires_grad_(True)
    yr = torch.where((y >= 0) & (y < K), y, torch.full_like(y, -100))
    l = F.cross_entropy(xr, yr, reduction="none", ignore_index=-100)
    sel, k = select(l.detach().reshape(-1), (yr != -100).reshape(-1), keep_ratio, min_kept, thresh)
    ws = (w.double()[yr.clamp_min(0)] if w is not None else torch.ones_like(l)) * sel.view_as(l)
    loss = (ws * l).sum() / ws.sum()
    return loss.detach(), torch.autograd.grad(loss, xr)[0], sel.view_as(l), k


def binary_reference(x, t, keep_ratio, min_kept, thresh):
    xr = x.detach().double().requires_grad_(True)
    l = F.binary_cross_entropy_with_logits(xr, t.double().view_as(xr), reduction="none")
    sel, k = select(l.detach().reshape(-1), torch.ones(l.numel(), dtype=torch.bool), keep_ratio, min_kept, thresh)
    loss = (l * sel.view_as(l)).sum() / sel.sum()
    return loss.detach(), torch.autograd.grad(loss, xr)[0], sel.view_as(l), k


def rel_l2(a, ref):
    a, ref = a.double().flatten().cpu(), ref.double().flatten().cpu()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()
