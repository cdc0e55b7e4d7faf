"""Inputs and the plain fp64 reference of the Lovasz tests (tests/test_lovasz_cpu.py, test_lovasz_gpu.py), written
from the paper (Berman et al., CVPR 2018): stable descending sort, cumulative intersection and union, J_i - J_{i-1},
torch autograd for the gradient.

Inputs come from a seeded CPU generator.  The gradient is discontinuous where two errors of a segment swap, so with
``min_gap`` the reference asserts -- it never skips -- that adjacent sorted fp64 errors of every segment differ by
more than that (the fp32 errors are good to about 1e-6).  GRAD_SEEDS were chosen on the CPU so that every gradient
case passes the assertion at 1e-5."""
import torch
import torch.nn.functional as F

N, H, W = 2, 17, 23   # the shape of tests/test_pixel_ce_gpu.py: partial blocks, ignored rows, one out-of-range label
GRAD_SHAPES = {2: (2, 13, 11), 3: (2, 13, 11), "hinge": (2, 13, 11), 5: (1, 5, 7), 21: (1, 5, 7)}
GRAD_SEEDS = {2: 1, 3: 3, "hinge": 1, 5: 1, 21: 1}
PATTERNS = ["digit0", "digit1", "digit2", "digit3", "equal", "zeros", "negzero", "nan", "invalid"]


def softmax_inputs(K, seed, shape=(N, H, W), absent=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, K, generator=g)   # class-last storage
    y = torch.randint(K, shape, generator=g)
    if absent:
        y[y == K - 1] = 0                     # the last class is in no label
    y[0, :3] = -100
    y[-1, -1, -1] = K + 3                     # out of range: ignored as well
    return x, y


def hinge_inputs(seed, shape=(N, H, W)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * 2, (torch.rand(*shape, generator=g) > 0.6).float()


def lovasz_grad(fg_sorted):
    """The paper's gradient of the Jaccard loss along the sorted errors: J_i - J_{i-1} (fg_sorted fp64 0 / 1)."""
    G = fg_sorted.sum()
    jac = 1 - (G - fg_sorted.cumsum(0)) / (G + (1 - fg_sorted).cumsum(0))
    out = jac.clone()
    out[1:] = jac[1:] - jac[:-1]
    return out


def closed_form(fg_sorted):
    """The same from the integer counts (bool fg_sorted): 1 / U, R / (U (U + 1)), 1 where U = 0; fp64."""
    fg = fg_sorted.long()
    G, Fb = fg.sum(), fg.cumsum(0) - fg
    U = (G + torch.arange(fg.numel()) - Fb).double()
    bg = torch.where(U == 0, torch.ones_like(U), (G - Fb).double() / (U * (U + 1)).clamp_min(1))
    return torch.where(fg_sorted, 1 / U.clamp_min(1), bg)


def segment_loss(e, fg, hinge=False, min_gap=None):
    es, perm = torch.sort(e, descending=True, stable=True)
    if min_gap is not None and es.numel() > 1:
        assert (es[:-1] - es[1:]).min() > min_gap, "two errors of a segment are too close"
    return ((es.clamp_min(0) if hinge else es) * lovasz_grad(fg[perm])).sum()


def _mean(v, like):
    return torch.stack(v).mean() if v else like.sum() * 0


def softmax_reference(x, y, classes="present", per_image=False, ce_weight=0.0, lovasz_weight=1.0, min_gap=None):
    """x fp32 [N, K, H, W] (any strides), y -> fp64 (loss, gradient)."""
    K = x.shape[1]
    xr = x.detach().double().requires_grad_(True)
    valid = (y >= 0) & (y < K)
    p = torch.softmax(xr, 1)
    per_sample = []
    for idx in ([slice(n, n + 1) for n in range(x.shape[0])] if per_image else [slice(None)]):
        v, segs = valid[idx], []
        for c in range(K):
            fg = (y[idx][v] == c).double()
            if classes == "all" or fg.sum() > 0:
                segs.append(segment_loss((fg - p[idx, c][v]).abs(), fg, False, min_gap))
        per_sample.append(_mean(segs, xr))
    loss = lovasz_weight * _mean(per_sample, xr)
    if ce_weight:
        loss = loss + ce_weight * F.cross_entropy(xr, torch.where(valid, y, torch.full_like(y, -100)))
    return loss.detach(), torch.autograd.grad(loss, xr)[0]


def hinge_reference(x, t, per_image=True, bce_weight=0.0, lovasz_weight=1.0, min_gap=None):
    """x fp32 [N, H, W], t float [N, H, W] -> fp64 (loss, gradient)."""
    xr = x.detach().double().requires_grad_(True)
    rows = x.shape[0] if per_image else 1
    xs, fg = xr.reshape(rows, -1), (t > 0.5).double().reshape(rows, -1)
    segs = [segment_loss(1 - xs[n] * (2 * fg[n] - 1), fg[n], True, min_gap) for n in range(rows)]
    loss = lovasz_weight * _mean(segs, xr)
    if bce_weight:
        loss = loss + bce_weight * F.binary_cross_entropy_with_logits(xr, t.double())
    return loss.detach(), torch.autograd.grad(loss, xr)[0]


def sort_case(name, S, L):
    """fp32 errors [S, L] whose bit patterns make one digit of the 8-bit x 4 radix sort decide, or hold ties, zeros,
    negatives with +-0, a NaN or invalid entries; fg and valid masks.  The S segments hold different data."""
    g = torch.Generator().manual_seed(7)
    r = torch.randint(0, 2 ** 31 - 1, (S, L), generator=g)
    u = torch.rand(S, L, generator=g)
    valid = torch.ones(S, L, dtype=torch.bool)
    if name == "digit0":
        err = (0x3F800000 | (r & 0xFF)).to(torch.int32).view(torch.float32)       # differ in bits 7..0 only
    elif name == "digit1":
        err = (0x3F800000 | (r & 0xFF00)).to(torch.int32).view(torch.float32)     # bits 15..8 only
    elif name == "digit2":
        err = (0x3F000000 | (r & 0xFF0000)).to(torch.int32).view(torch.float32)   # bits 23..16 only
    elif name == "digit3":
        top = r % 200 + 20                                                          # bits 31..24 only, finite
        err = ((top << 24) - ((top >> 7) << 32)).to(torch.int32).view(torch.float32)
    elif name == "equal":
        err = torch.ones(S, L)
    else:
        err = torch.rand(S, L, generator=g)
        if name == "zeros":
            err[u < 0.6] = 0.0
        elif name == "negzero":                                                     # the hinge form's range
            err = err * 4 - 2
            err[u < 0.2] = 0.0
            err[(u >= 0.2) & (u < 0.4)] = -0.0
        elif name == "nan":
            err[:, L // 2] = float("nan")
        elif name == "invalid":
            valid = u >= 0.3
    return err, torch.rand(S, L, generator=g) < 0.4, valid


def check_sort(be, dev, name, S, L):
    """The backend's lovasz_sort on sort_case: the permutation of the valid prefix equals torch's stable descending
    sort, g is within 1e-6 (relative) of the fp64 closed form at that permutation, invalid entries get exactly 0."""
    err, fg, valid = sort_case(name, S, L)
    perm, g, seg_loss = (t.cpu() for t in be.lovasz_sort(err.to(dev), fg.to(dev), valid.to(dev), hinge=True))
    for s in range(S):
        vi = valid[s].nonzero().flatten()
        want = vi[torch.sort(err[s][vi], descending=True, stable=True).indices]
        assert torch.equal(perm[s, : vi.numel()], want), (name, S, L, s)
        gr = closed_form(fg[s][want])
        assert ((g[s][want].double() - gr).abs() <= 1e-6 * gr.abs()).all(), (name, S, L, s)
        assert (g[s][~valid[s]] == 0).all()
        if name != "nan":
            lr = (err[s][want].double().clamp_min(0) * gr).sum()
            assert abs(seg_loss[s].item() - lr.item()) < 1e-4 * max(1.0, abs(lr.item())), (name, S, L, s)


def rel_l2(a, ref):
    a, ref = a.double().flatten().cpu(), ref.double().flatten().cpu()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()
