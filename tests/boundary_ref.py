"""Inputs and the plain references of the boundary-loss tests (tests/test_boundary_cpu.py, test_boundary_gpu.py): the
Euclidean distance transform by brute force (the int64 minimum over all seed pixels), the signed map formed from those
integers in fp64 (Kervadec et al., MIDL 2019, ``one_hot2dist``), and the loss written from its definition in fp64 with
torch autograd for the gradient.  Inputs come from a seeded CPU generator; references are computed once per process."""
import functools

import torch
import torch.nn.functional as F

N, H, W = 2, 37, 70   # two strips of the column pass, two segments of the row pass, partial blocks
INF = 2 ** 31 - 1
PATTERNS = ["empty", "full", "corner", "corner_complement", "checker", "random001", "random05", "diagonal"]


def edt_shapes(strip, strip_rows):
    """(H, W): the degenerate ones, the base shape, the widths around the strip, one row past the strip's halving."""
    return [(1, 1), (1, 70), (70, 1), (H, W), (5, strip - 1), (5, strip), (5, strip + 1), (strip_rows + 1, 33)]


def mask_case(name, h, w):
    g = torch.Generator().manual_seed(h * 1000 + w)
    m = torch.zeros(h, w, dtype=torch.bool)
    if name in ("corner", "corner_complement"):
        m[h - 1, w - 1] = True           # the longest scan from (0, 0)
    elif name == "checker":
        m = (torch.arange(h)[:, None] + torch.arange(w)[None, :]) % 2 == 0
    elif name.startswith("random"):
        m = torch.rand(h, w, generator=g) < (0.01 if name == "random001" else 0.5)
    elif name == "diagonal":
        m[torch.arange(h), torch.arange(h) * w // h] = True
    return ~m if name in ("full", "corner_complement") else m


def brute_edt(mask):
    """bool [h, w] -> int64 [h, w]: min over the True pixels s of |q - s|^2, INF without one."""
    h, w = mask.shape
    seeds = mask.nonzero()
    if seeds.numel() == 0:
        return torch.full((h, w), INF, dtype=torch.int64)
    q = torch.stack(torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij"), -1).reshape(-1, 2)
    out = torch.empty(h * w, dtype=torch.int64)
    step = max(1, (1 << 23) // seeds.shape[0])
    for i in range(0, h * w, step):
        out[i:i + step] = ((q[i:i + step, None] - seeds[None]) ** 2).sum(-1).min(1).values
    return out.view(h, w)


@functools.lru_cache(maxsize=None)
def edt_case(name, h, w):
    m = mask_case(name, h, w)
    return m, brute_edt(m).to(torch.int32)


def signed_reference(member):
    """bool [..., h, w] -> fp64 phi from the exact integers: +sqrt(d2_in) outside, 1 - sqrt(d2_out) inside, 0 for an
    empty or image-filling set."""
    flat = member.reshape(-1, *member.shape[-2:])
    out = torch.empty(flat.shape, dtype=torch.float64)
    for i, m in enumerate(flat):
        d_in, d_out = brute_edt(m), brute_edt(~m)
        phi = torch.where(m, 1 - d_out.double().sqrt(), d_in.double().sqrt())
        out[i] = torch.where(torch.where(m, d_out, d_in) == INF, torch.zeros_like(phi), phi)
    return out.view(member.shape)


def members(y, K):
    return y.unsqueeze(1) == torch.arange(K).view(1, K, 1, 1)   # ignored / out-of-range labels are in no class


def check_signed_map(phi, ref):
    """phi fp32 against float32(ref) to 1 ulp, exactly 0 where the reference is."""
    r32 = ref.to(torch.float32)
    ulp = torch.ldexp(torch.ones_like(r32), torch.frexp(r32).exponent - 24)
    assert ((phi.cpu() - r32).abs() <= ulp).all() and (phi.cpu()[ref == 0] == 0).all()


@functools.lru_cache(maxsize=None)
def softmax_inputs(K, seed, absent=True):
    """Class-last logits [N, H, W, K] and labels in 6 x 6 blocks (distances of several pixels), the last class in no
    label, three ignored rows and one out-of-range label."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, K, generator=g)
    y = torch.randint(K, (N, H // 6 + 1, W // 6 + 1), generator=g)
    y = y.repeat_interleave(6, 1).repeat_interleave(6, 2)[:, :H, :W].contiguous()
    if absent:
        y[y == K - 1] = 0
    y[0, :3] = -100
    y[-1, -1, -1] = K + 3
    return x, y, signed_reference(members(y, K))


@functools.lru_cache(maxsize=None)
def sigmoid_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, generator=g) * 2
    t = (torch.rand(N, H // 6 + 1, W // 6 + 1, generator=g) > 0.6).float()
    t = t.repeat_interleave(6, 1).repeat_interleave(6, 2)[:, :H, :W].contiguous()
    return x, t, signed_reference(t > 0.5)


def softmax_reference(x, y, phi, include_background=True, ce_weight=0.0, boundary_weight=1.0):
    """x [N, K, H, W] (any strides), y, phi fp64 [N, K, H, W] -> fp64 (loss, gradient)."""
    K = x.shape[1]
    xr = x.detach().double().requires_grad_(True)
    valid = (y >= 0) & (y < K)
    c0 = 0 if include_background else 1
    term = (torch.softmax(xr, 1) * phi)[:, c0:] * valid.unsqueeze(1)
    nv = valid.sum()
    loss = boundary_weight * (term.sum() / (nv * (K - c0)) if nv > 0 else term.sum() * 0)
    if ce_weight:
        loss = loss + ce_weight * F.cross_entropy(xr, torch.where(valid, y, torch.full_like(y, -100)))
    return loss.detach(), torch.autograd.grad(loss, xr)[0]


def sigmoid_reference(x, t, phi, bce_weight=0.0, boundary_weight=1.0):
    xr = x.detach().double().requires_grad_(True)
    loss = boundary_weight * (torch.sigmoid(xr) * phi).mean()
    if bce_weight:
        loss = loss + bce_weight * F.binary_cross_entropy_with_logits(xr, t.double())
    return loss.detach(), torch.autograd.grad(loss, xr)[0]


def rel_l2(a, ref):
    a, ref = a.double().flatten().cpu(), ref.double().flatten().cpu()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()
