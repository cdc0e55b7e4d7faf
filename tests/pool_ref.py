"""fp64 reference of the pool / resample / layout / head-gradient family (csrc/kernels/pool.hip, the two
fused gradient producers of head.hip, pixel_ce.hip's pad-cast) -- explicit formulas in plain torch,
written from the definitions of the operations, not from the kernels' code.

Every function takes tensors of any floating type (and device) and returns fp64 unless it says otherwise
(indices: uint8; the functions that only select or copy values take ``dtype`` to work in another
type, which is still exact).  Activations are NHWC ``[N, H, W, C]``.  tests/test_pool_ref_cpu.py ties
these formulas to torch (max_pool2d, interpolate, adaptive_avg_pool2d, permute + pad, autograd) in fp64.
"""
import torch

from bn_ref import F64, U, d, mask_bits, store_tol   # noqa: F401  (re-exported: one vocabulary of bounds)


def out_size(n, k, s, p):
    """Floor mode: the windows that start inside the padded extent and fit in it."""
    return (n + 2 * p - k) // s + 1


# ------------------------------------------------------------------ max pool
def maxpool(x, k, s, p, dtype=F64):
    """(y [N, OH, OW, C], idx uint8): the maximum over the in-image taps of each k x k window and
    idx = kh*k + kw of the first maximum in (kh, kw) scan order.  Out-of-image taps never take part; a
    NaN wins over any number and the first NaN stays; a window with no value above -inf reports its
    first in-image tap."""
    x = x.to(dtype)
    N, H, W, C = x.shape
    OH, OW = out_size(H, k, s, p), out_size(W, k, s, p)
    dev = x.device
    oh, ow = torch.arange(OH, device=dev) * s - p, torch.arange(OW, device=dev) * s - p
    best = torch.full((N, OH, OW, C), float("-inf"), dtype=dtype, device=dev)
    idx = torch.zeros((N, OH, OW, C), dtype=torch.uint8, device=dev)
    seen = torch.zeros((1, OH, OW, 1), dtype=torch.bool, device=dev)   # a tap of the window was in the image
    for kh in range(k):
        for kw in range(k):
            ih, iw = oh + kh, ow + kw
            inside = ((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None, :]
            inside = inside[None, :, :, None]
            v = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
            take = inside & (~seen | (v > best) | (v.isnan() & ~best.isnan()))
            best = torch.where(take, v, best)
            idx = torch.where(take, torch.full_like(idx, kh * k + kw), idx)
            seen = seen | inside
    return best, idx


def maxpool_bwd_terms(dy, idx, H, W, k, s, p, add=None, dtype=F64):
    """(dx [N, H, W, C], sum of the absolute terms): every output gradient goes to the input element
    its stored index names (a scatter-add), plus ``add`` (a second gradient of the pool input)."""
    dy = dy.to(dtype)
    N, OH, OW, C = dy.shape
    dev = dy.device
    i = idx.long()
    ih = (torch.arange(OH, device=dev) * s - p)[None, :, None, None] + i // k
    iw = (torch.arange(OW, device=dev) * s - p)[None, None, :, None] + i % k
    assert bool(((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).all()), "an index names an out-of-image tap"
    n = torch.arange(N, device=dev)[:, None, None, None]
    c = torch.arange(C, device=dev)[None, None, None, :]
    flat = (((n * H + ih) * W + iw) * C + c).reshape(-1)
    dx = torch.zeros(N * H * W * C, dtype=dtype, device=dev).index_add_(0, flat, dy.reshape(-1))
    mag = torch.zeros(N * H * W * C, dtype=dtype, device=dev).index_add_(0, flat, dy.abs().reshape(-1))
    dx, mag = dx.view(N, H, W, C), mag.view(N, H, W, C)
    if add is not None:
        dx, mag = dx + add.to(dtype), mag + add.to(dtype).abs()
    return dx, mag


def maxpool_bwd(dy, idx, H, W, k, s, p, add=None, dtype=F64):
    return maxpool_bwd_terms(dy, idx, H, W, k, s, p, add, dtype)[0]


def apply_relu(z, scale, shift, dtype):
    """relu(z*scale + shift) rounded to the storage type: the pooled input of the fused forward."""
    return (d(z) * d(scale) + d(shift)).clamp_min(0.0).to(dtype).to(F64)


def relu_mask(z, scale, shift):
    """[z*scale + shift > 0]: the elements a gradient of relu(BN(z)) passes through."""
    return d(z) * d(scale) + d(shift) > 0


# ------------------------------------------------------------------ global average pool
def avgpool_terms(x):
    """x [N, HW, C] -> (mean over HW [N, C], sum |x| / HW)."""
    x = d(x)
    return x.mean(1), x.abs().mean(1)


def avgpool(x):
    return avgpool_terms(x)[0]


def avgpool_bwd(dy, HW):
    """dy [N, C] -> [N, HW, C]: every pixel gets dy / HW."""
    dy = d(dy)
    return (dy / HW)[:, None, :].expand(dy.shape[0], HW, dy.shape[1])


# ------------------------------------------------------------------ bilinear x2, align_corners=True
def _bilinear2x_taps(n):
    """Output index o reads the input at o (n-1)/(2n-1): (floor, fraction) from integer arithmetic."""
    o = torch.arange(2 * n, dtype=torch.int64)
    num, den = o * (n - 1), 2 * n - 1
    i0 = num // den
    return i0, (i0 + 1).clamp_max(n - 1), (num % den).to(F64) / den


def bilinear2x_matrix(n, device="cpu"):
    """[2n, n] fp64: row o interpolates linearly between the two inputs around o (n-1)/(2n-1) (exact
    rational coordinates); n = 1: all ones."""
    i0, i1, f = _bilinear2x_taps(n)
    A = torch.zeros(2 * n, n, dtype=F64)
    r = torch.arange(2 * n)
    A[r, i0] += 1.0 - f
    A[r, i1] += f
    return A.to(device)


def bilinear2x_footprint(n, device="cpu"):
    """[2n, n] fp64 of 0 / 1: the inputs row o of the matrix may read (both neighbours of its coordinate)."""
    i0, i1, _ = _bilinear2x_taps(n)
    Fp = torch.zeros(2 * n, n, dtype=F64)
    r = torch.arange(2 * n)
    Fp[r, i0] = 1.0
    Fp[r, i1] = 1.0
    return Fp.to(device)


def _sep(Ah, x, Aw):
    return torch.einsum("oh,nhwc,pw->nopc", Ah, x, Aw)


def _sep_t(Ah, g, Aw):
    return torch.einsum("oh,nopc,pw->nhwc", Ah, g, Aw)


def upsample(x):
    """x [N, H, W, C] -> [N, 2H, 2W, C] = A_h x A_w^T per channel."""
    x = d(x)
    return _sep(bilinear2x_matrix(x.shape[1], x.device), x, bilinear2x_matrix(x.shape[2], x.device))


def upsample_bwd(g):
    """g [N, 2H, 2W, C] -> [N, H, W, C] = A_h^T g A_w: the transpose of upsample by construction."""
    g = d(g)
    return _sep_t(bilinear2x_matrix(g.shape[1] // 2, g.device), g, bilinear2x_matrix(g.shape[2] // 2, g.device))


def upsample_terms(x):
    """(sum |w_i x_i|, sum of |x| over the 2 x 2 footprint) per output element."""
    x = d(x).abs()
    H, W, dev = x.shape[1], x.shape[2], x.device
    return (_sep(bilinear2x_matrix(H, dev), x, bilinear2x_matrix(W, dev)),
            _sep(bilinear2x_footprint(H, dev), x, bilinear2x_footprint(W, dev)))


def upsample_bwd_terms(g):
    """(sum |w_i g_i|, sum of |g| over the outputs whose footprint holds the element, their number)."""
    g = d(g).abs()
    H, W, dev = g.shape[1] // 2, g.shape[2] // 2, g.device
    Fh, Fw = bilinear2x_footprint(H, dev), bilinear2x_footprint(W, dev)
    count = Fh.sum(0)[:, None] * Fw.sum(0)[None, :]
    return (_sep_t(bilinear2x_matrix(H, dev), g, bilinear2x_matrix(W, dev)), _sep_t(Fh, g, Fw),
            count[None, :, :, None])


# ------------------------------------------------------------------ layouts
def nchw_to_nhwc_pad(x, Cpad, dtype=F64):
    """x [N, C, H, W] -> [N, H, W, Cpad], channels C.. zero."""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, Cpad, dtype=dtype, device=x.device)
    y[..., :C] = x.to(dtype).permute(0, 2, 3, 1)
    return y


def s2d(x, pad, U_, V, CS, dtype=F64):
    """2x2 space-to-depth of the zero-padded image: y[n][u][v][(vh*2 + vw)*CS + c] =
    x[n][c][2u + vh - pad][2v + vw - pad], zero outside the image and for c >= C.  One loop per slot."""
    N, C, H, W = x.shape
    dev = x.device
    y = torch.zeros(N, U_, V, 4 * CS, dtype=dtype, device=dev)
    xs = x.to(dtype).permute(0, 2, 3, 1)
    for vh in (0, 1):
        for vw in (0, 1):
            h, w = 2 * torch.arange(U_, device=dev) + vh - pad, 2 * torch.arange(V, device=dev) + vw - pad
            inside = ((h >= 0) & (h < H))[:, None] & ((w >= 0) & (w < W))[None, :]
            v = xs[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)]
            slot = vh * 2 + vw
            y[..., slot * CS:slot * CS + C] = torch.where(inside[None, :, :, None], v, torch.zeros_like(v))
    return y


def pad_cast(x, Kp, dtype=F64):
    """x [M, K] -> [M, Kp], columns K.. zero."""
    M, K = x.shape
    y = torch.zeros(M, Kp, dtype=dtype, device=x.device)
    y[:, :K] = x.to(dtype)
    return y


# ------------------------------------------------------------------ the fused gradient producers
def masked_sums(dx_stored, z):
    """The BN-backward partials of a stored masked gradient: (sums [2][C] = sum dx, sum dx*z; the sums
    of the absolute terms).  dx_stored, z: [M, C]."""
    g, z = d(dx_stored), d(z)
    gz = g * z
    return torch.stack([g.sum(0), gz.sum(0)]), torch.stack([g.abs().sum(0), gz.abs().sum(0)])


def head_dgrad_terms(dl, w, z, scale, shift):
    """(dx, sum_k |dl_k w_k|) of the masked data gradient of a 1x1 convolution with K outputs."""
    dl, w = d(dl), d(w)
    m = relu_mask(z, scale, shift)
    zero = torch.zeros((), dtype=F64, device=dl.device)
    return torch.where(m, dl @ w.t(), zero), torch.where(m, dl.abs() @ w.abs().t(), zero)


def head_dgrad(dl, w, z, scale, shift, dtype=None):
    """dl [M, K], w [C, K], z [M, C]: dx[m, c] = [z*scale + shift > 0] sum_k dl[m, k] w[c, k] (K = 1: the
    outer product) -> (dx, sums [2][C], abs-sums); the sums are those of dx rounded to ``dtype``."""
    dx = head_dgrad_terms(dl, w, z, scale, shift)[0]
    sums, mags = masked_sums(dx if dtype is None else dx.to(dtype), z)
    return dx, sums, mags
