"""Cases and the brute-force fp64 reference of the surface-distance tests (tests/test_surface_cpu.py,
test_surface_gpu.py).  The reference shares nothing with RefBackend: edges by explicit neighbour comparison on a map
padded with "no class", distances as the minimum over torch.cdist of integer coordinates (squared and rounded to the
integer they are), the order statistic by numpy.percentile(method="linear") on the fp64 roots.

A case is (N, K, H, W, how the maps are made, percentile); K = 0 is the binary form with logits [N, H, W], K = 1 the
binary form with logits [N, 1, H, W].  TILE is the edge pass's tile (asserted by the GPU test to be the backend's)."""
import functools

import numpy as np
import torch

TILE = 32
IGNORE = -100
CASES = [
    (2, 3, TILE + 1, TILE + 1, "blocks", 95.0),      # one pixel past a tile in both directions: seams and halo
    (1, 2, TILE + 1, 2 * TILE + 1, "blocks", 50.0),
    (1, 21, 37, 70, "blocks", 95.0),
    (1, 3, TILE + 1, TILE + 1, "blocks", 100.0),     # column 1 is column 0
    (1, 3, TILE + 1, TILE + 1, "ties", 95.0),        # exact ties between logits: the lowest index wins
    (1, 3, 1, 40, "blocks", 95.0),                   # H = 1: every pixel is an edge pixel
    (1, 3, 40, 1, "blocks", 50.0),
    (1, 3, TILE + 1, TILE + 1, "identical", 95.0),   # pred = gt: all zeros
    (1, 4, 20, 20, "absent", 95.0),                  # class 1 in gt only, 2 in pred only, 3 in neither: inf, inf, NaN
    (1, 2, 9, 12, "dots", 50.0),                     # one pixel in a corner (m = 1) against two pixels (m = 2, t = 0.5)
    (1, 2, 40, 40, "checker", 95.0),                 # 800 items in a list, heavy ties
    (2, 0, TILE + 1, TILE + 1, "blocks", 95.0),
    (2, 1, TILE + 1, TILE + 1, "blocks", 50.0),
    (3, 0, 8, 8, "absent", 95.0),                    # binary: pred empty, gt empty, both empty
]


def _blocks(g, n, k, h, w):
    y = torch.randint(k, (n, h // 6 + 1, w // 6 + 1), generator=g)
    return y.repeat_interleave(6, 1).repeat_interleave(6, 2)[:, :h, :w].contiguous()


def class_maps(N, K, H, W, how, seed=0):
    """-> (pred, gt) int64 [N, H, W] over max(K, 2) classes; gt may hold IGNORE and out-of-range labels."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    kk = max(K, 2)
    pred, gt = torch.zeros(N, H, W, dtype=torch.int64), torch.zeros(N, H, W, dtype=torch.int64)
    if how in ("blocks", "ties", "identical"):
        gt = _blocks(g, N, kk, H, W)
        pred = gt.clone() if how == "identical" else _blocks(g, N, kk, H, W)
        if K >= 2 and how != "identical" and H > 8:
            gt[0, 3:6] = IGNORE          # a band of ignored pixels
            gt[-1, -1, -1] = K + 3       # an out-of-range label
    elif how == "absent" and K >= 2:
        gt[0, 4:9, 4:9], pred[0, 10:15, 3:12] = 1, 2
    elif how == "absent":
        gt[0, 2:5, 2:5], pred[1, 3:6, 1:4] = 1, 1
    elif how == "dots":
        pred[0, 0, 0] = 1
        gt[0, 4, 5:7] = 1
    elif how == "checker":
        pred = ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2).expand(N, H, W).contiguous()
        gt = pred.clone()
        gt[:, :, W // 2:] = 0
    return pred, gt


@functools.lru_cache(maxsize=None)
def inputs(N, K, H, W, how, seed=0):
    """-> (logits class-last fp32 [N, H, W, K] or [N, H, W], target int64 labels or the float target)."""
    pred, gt = class_maps(N, K, H, W, how, seed)
    g = torch.Generator().manual_seed(seed + 7)
    if K < 2:
        return torch.where(pred > 0, 1.0, -1.0) * (0.5 + torch.rand(N, H, W, generator=g)), (gt > 0).float()
    x = torch.rand(N, H, W, K, generator=g)
    x.scatter_(3, pred.unsqueeze(3), 2.0)
    if how == "ties":   # every class above pred ties with it at the maximum
        x = torch.where(torch.arange(K).view(1, 1, 1, K) > pred.unsqueeze(3), torch.full_like(x, 2.0), x)
    return x, gt


def _edges(m):
    """int64 [H, W] (-1: no class) -> bool [H, W]: in a class and a 4-neighbour (or the border) is not in it."""
    p = np.pad(m, 1, constant_values=-1)
    c = p[1:-1, 1:-1]
    out = (p[:-2, 1:-1] != c) | (p[2:, 1:-1] != c) | (p[1:-1, :-2] != c) | (p[1:-1, 2:] != c)
    return (c >= 0) & out


def _d2(a, b):
    """edge masks -> int64 [|a|]: the squared distance of every pixel of a to the nearest pixel of b."""
    qa, qb = (torch.from_numpy(np.argwhere(m)).double() for m in (a, b))
    return torch.cdist(qa, qb).min(1).values.square().round().long().numpy()


@functools.lru_cache(maxsize=None)
def reference(N, K, H, W, how, percentile, seed=0):
    """-> (metrics fp64 [N, max(K, 1), 3], counts int64 [N, max(K, 1), 2]) of the case, from the definition."""
    x, t = inputs(N, K, H, W, how, seed)
    if K < 2:
        pm, gm, kk = np.where(x.numpy() > 0, 0, -1), np.where(t.numpy() > 0.5, 0, -1), 1
    else:
        valid = ((t != IGNORE) & (t >= 0) & (t < K)).numpy()
        pm, gm, kk = np.where(valid, x.numpy().argmax(3), -1), np.where(valid, t.numpy(), -1), K   # argmax: the first
    metrics, counts = np.full((N, kk, 3), np.nan), np.zeros((N, kk, 2), dtype=np.int64)
    for n in range(N):
        for c in range(kk):
            P, G = _edges(np.where(pm[n] == c, c, -1)), _edges(np.where(gm[n] == c, c, -1))
            counts[n, c] = P.sum(), G.sum()
            if not (P.any() and G.any()):
                metrics[n, c] = np.inf if (P.any() or G.any()) else np.nan
                continue
            d = [np.sqrt(_d2(P, G).astype(np.float64)), np.sqrt(_d2(G, P).astype(np.float64))]
            metrics[n, c] = (max(v.max() for v in d),
                             max(np.percentile(v, percentile, method="linear") for v in d),
                             (d[0].sum() + d[1].sum()) / (len(d[0]) + len(d[1])))
    return torch.from_numpy(metrics), torch.from_numpy(counts)


def device_inputs(case, device, layout="nchw"):
    """The case's (logits, target) on ``device``; layout nchw or nhwc_view (the engine's NHWC buffer seen as NCHW)."""
    N, K, H, W, how, _ = case
    x, t = inputs(N, K, H, W, how)
    x = x.to(device)
    if K >= 2:
        x = x.permute(0, 3, 1, 2)
        x = x if layout == "nhwc_view" else x.contiguous()
    elif K == 1:
        x = x.unsqueeze(1)
    return x, t.to(device)


def check(metrics, counts, case):
    """counts equal; NaN and inf where the reference has them; column 0 the bits of float32(reference); columns 1
    and 2 within one fp32 ulp of float32(reference); at percentile 100 column 1 is column 0, bit for bit."""
    N, K, H, W, how, p = case
    ref, rc = reference(N, K, H, W, how, p)
    metrics, r32 = metrics.cpu(), ref.to(torch.float32)
    assert metrics.dtype == torch.float32 and counts.dtype == torch.int64
    assert torch.equal(counts.cpu(), rc)
    fin = torch.isfinite(r32)
    assert torch.equal(torch.isnan(metrics), torch.isnan(r32)) and torch.equal(torch.isinf(metrics), torch.isinf(r32))
    assert (metrics[~fin & ~torch.isnan(r32)] > 0).all()
    m, r = metrics[fin].view(-1, 3), r32[fin].view(-1, 3)
    ulp = torch.ldexp(torch.ones_like(r), torch.frexp(r).exponent - 24)
    print(f"{case}: max |d| / ulp per column {((m - r).abs() / ulp).amax(0).tolist() if len(m) else []}")
    assert torch.equal(m[:, 0], r[:, 0])
    assert ((m - r).abs() <= ulp).all()
    if p == 100.0:
        assert torch.equal(m[:, 1], m[:, 0])
    return m
