"""The pool / resample / layout / head-gradient kernels (csrc/kernels/pool.hip, outer_dgrad_bn and
head_dgrad_bn of head.hip, nhwc_pad_cast of pixel_ce.hip) against the fp64 reference of tests/pool_ref.py
at their edge shapes: both max-pool forward kernels and every window extent of the backward, odd sizes,
ties, NaN, -inf, channel slices of every operand that takes ld / off, every row map of the fused
producers, the candidate range of the bilinear backward, the second trip of the capped grids, the
launchers' refusals.

Comparisons are elementwise, of the kernel's stored output with fp64 computed on the device from the
SAME stored inputs; every output (and every buffer wider than its slice) starts as a sentinel.  What
only selects or copies (max pool, layouts, masks) must be exact; the bounds of the rest count roundings
(profiles/pool_tests/README.md derives each), u = 2^-24, h = half a bf16 ulp of ref (0 for fp32):

* max-pool backward   h + n u sum|terms|, n = ceil(k/s)^2 (+ 1 with add)
* fused partials      |sum_blocks partial - ref| <= (L + r) u sum|term| per channel, ref over the stored dx
* head gradients      h + K u sum_k |dl_k w_k|
* average pool        h + (HW + 2) u sum|x| / HW forward, h + 2 u |ref| backward
* bilinear x2         h + k u sum|w_i x_i| + (dH + dW + dH dW) F, k = 6 forward and 6 + T backward, dn = 2 u (n - 1)
                      the coordinate error, F the sum of |x| over the footprint, T its number of terms

Masks are decided on a dyadic fill (multiples of 1/8, scale +-{1/2, 1, 2}, shift in eighths) on which
z*scale + shift is exact in fp32: no element is excused anywhere.
"""
import math
import zlib

import pytest
import torch

import pool_ref as R
from deeplearning_mpi_amd.ops.backend import NativeBackend

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
FILLS = ["dyadic", "randn"]
SENT = 640.0   # exact in bf16; no kernel output below comes near it
ISENT = 255    # no window position: k <= 15 in every case


@pytest.fixture(scope="module")
def nb():
    return NativeBackend(DEV)


def _gen(*seed):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(seed).encode()))


def _dyadic(shape, g, zeros=0.4):
    """Multiples of 1/8 in [-4, 4] with a share of exact zeros: tie-rich, exact in bf16."""
    v = torch.randint(-32, 33, shape, generator=g, device=DEV).float() / 8
    if zeros:
        v[torch.rand(shape, generator=g, device=DEV) < zeros] = 0.0
    return v


def _fill(kind, shape, g, zeros=0.4):
    return _dyadic(shape, g, zeros) if kind == "dyadic" else torch.randn(shape, generator=g, device=DEV)


def _bn_coef(C, g):
    """scale in +-{1/2, 1, 2}, shift in eighths (every third exactly 0): z*scale + shift is exact in fp32."""
    scale = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (C,), generator=g, device=DEV)]
    scale = scale * (torch.randint(0, 2, (C,), generator=g, device=DEV).float() * 2 - 1)
    shift = torch.randint(-8, 9, (C,), generator=g, device=DEV).float() / 8
    shift[0::3] = 0.0
    return scale, shift


def _slab(values, ld, off, dtype):
    """values [..., C] stored as the channel slice [off, off + C) of a [rows, ld] buffer of sentinels."""
    C = values.shape[-1]
    assert ld % 8 == 0 and off % 8 == 0 and off + C <= ld
    buf = torch.full((values.numel() // C, ld), SENT, device=DEV, dtype=dtype)
    buf[:, off:off + C] = values.reshape(-1, C).to(dtype)
    return buf


def _out(rows, C, ld, off, dtype):
    """An output slab: sentinels everywhere, so an unwritten element fails."""
    return torch.full((rows, ld), SENT, device=DEV, dtype=dtype)


def _cut(buf, off, C, shape):
    return buf[:, off:off + C].reshape(*shape, C)


def _outside_untouched(buf, off, C):
    keep = torch.ones(buf.shape[1], dtype=torch.bool, device=buf.device)
    keep[off:off + C] = False
    return bool((buf[:, keep] == SENT).all())


def _le(err, tol):
    """err <= tol everywhere (a NaN on either side fails)."""
    return bool((err <= tol).all())


def _worst(err, tol):
    r = torch.nan_to_num(err / tol.clamp_min(1e-300), nan=float("inf"))
    return f"worst err / bound = {r.max().item():.3g} at {tuple(int(i) for i in (r == r.max()).nonzero()[0])}"


def _same(a, b):
    """Equal values; NaN equals NaN (the NaN cases), +-0 compare equal."""
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def _bits_equal(y, ref_f32):
    """y equals ref (fp32 values) stored in y's type, bit for bit: padding zeros are +0.0."""
    if y.dtype == F32:
        return torch.equal(y.view(torch.int32), ref_f32.view(torch.int32))
    return torch.equal(y.view(torch.int16), ref_f32.to(BF16).view(torch.int16))


# ------------------------------------------------------------------ max pool: the calls
def _osz(H, W, k, s, p):
    return R.out_size(H, k, s, p), R.out_size(W, k, s, p)


def _mp_fwd(nb, xbuf, N, H, W, C, ldx, xoff, k, s, p, bn=None, ys=None, ldys=0, ysoff=0):
    """-> (y [N, OH, OW, C], idx uint8 [N, OH, OW, C]); both start as sentinels."""
    OH, OW = _osz(H, W, k, s, p)
    y = _out(N * OH * OW, C, C, 0, xbuf.dtype)
    idx = torch.full((N * OH * OW * C,), ISENT, dtype=torch.uint8, device=DEV)
    sc, sh = bn if bn is not None else (None, None)
    nb.C.maxpool_fwd(xbuf, N, H, W, C, ldx, xoff, k, s, p, y, idx, OH, OW, sc, sh, ys, ldys, ysoff)
    return y.view(N, OH, OW, C), idx.view(N, OH, OW, C)


def _check_fwd(nb, vals, k, s, p, dtype, ld=None, off=0, bn=None, store=None, what=""):
    """vals [N, H, W, C] fp32 (exact in the storage type or rounded to it here) -> the kernel's (y, idx)."""
    N, H, W, C = vals.shape
    ld = C if ld is None else ld
    xbuf = _slab(vals, ld, off, dtype)
    x = _cut(xbuf, off, C, (N, H, W))
    ys = None
    if store is not None:
        ys = _out(N * H * W, C, store[0], store[1], dtype)
    y, idx = _mp_fwd(nb, xbuf, N, H, W, C, ld, off, k, s, p, bn, ys, *(store or (0, 0)))
    pooled = x if bn is None else R.apply_relu(x, bn[0], bn[1], dtype)
    yr, ir = R.maxpool(pooled, k, s, p)
    assert _same(y.double(), yr), f"{what}: y differs from the reference"
    assert torch.equal(idx, ir), f"{what}: idx differs at {int((idx != ir).sum())} elements"
    assert _outside_untouched(xbuf, off, C)
    if store is not None:
        assert torch.equal(_cut(ys, store[1], C, (N, H, W)).double(), pooled), f"{what}: ys"
        assert _outside_untouched(ys, store[1], C), f"{what}: ys wrote outside its slice"
    return y, idx


#          k  s  p   N  H   W   C
FIXED = [(3, 2, 1, 2, 7, 9, 8), (3, 2, 1, 1, 1, 1, 8), (3, 2, 1, 1, 2, 3, 24),
         (2, 2, 0, 2, 8, 6, 8), (2, 2, 0, 1, 7, 5, 40), (2, 2, 0, 2, 16, 24, 128)]
RUNTIME = [(3, 1, 1, 1, 5, 6, 16), (2, 1, 0, 2, 4, 5, 8), (3, 3, 0, 1, 9, 7, 8), (5, 2, 2, 1, 9, 11, 8),
           (3, 2, 0, 1, 8, 8, 16), (4, 2, 1, 1, 10, 6, 8)]
SLICED = (3, 2, 1, 2, 16, 16, 64)   # x is the slice ld 192, off 128
GEOMS = FIXED + [SLICED] + RUNTIME


def _id(c):
    return "k{}s{}p{}-{}x{}x{}x{}".format(*c)


# ------------------------------------------------------------------ max pool forward
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GEOMS, ids=_id)
def test_maxpool_fwd(nb, case, dtype, fill):
    """Values and indices exact: both fixed kernels, the runtime-k kernel, odd sizes, H = 1, ties."""
    k, s, p, N, H, W, C = case
    ld, off = (192, 128) if case == SLICED else (C, 0)
    _check_fwd(nb, _fill(fill, (N, H, W, C), _gen(*case, fill)), k, s, p, dtype, ld, off, what=_id(case))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,store", [((2, 2, 0, 2, 8, 6, 24), (64, 8)), ((3, 2, 1, 2, 7, 9, 8), None),
                                        ((3, 1, 1, 1, 5, 6, 16), None)], ids=["k2-store", "k3", "runtime"])
def test_maxpool_fwd_fused_bn(nb, case, store, dtype):
    """bn=: the pooled input is the storage rounding of relu(fma(z, scale, shift)); store=: it is also
    written to ys (ldys 64, ysoff 8)."""
    k, s, p, N, H, W, C = case
    g = _gen(*case, "bn")
    _check_fwd(nb, _dyadic((N, H, W, C), g), k, s, p, dtype, bn=_bn_coef(C, g), store=store, what=_id(case))


@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool_special_values(nb, dtype):
    """3x3/s2/p1 on (2,7,9,8): padding never wins; a NaN wins and the first NaN stays; a border window of
    -inf alone names an in-image tap and the backward delivers its gradient there."""
    k, s, p, N, H, W, C = 3, 2, 1, 2, 7, 9, 8
    g = _gen(dtype == BF16, "special")
    x = -1.0 - _dyadic((N, H, W, C), g).abs()
    y, _ = _check_fwd(nb, x, k, s, p, dtype, what="all <= -1")
    assert bool((y < 0).all()) and bool(torch.isfinite(y).all())

    x = _fill("randn", (N, H, W, C), g)
    x[0, 1, 1, :] = float("nan")                      # in four windows: their taps 8, 6, 2 and 0
    y, idx = _check_fwd(nb, x, k, s, p, dtype, what="one NaN")
    assert bool(y[0, :2, :2].isnan().all()) and int(y.isnan().sum()) == 4 * C
    assert bool((idx[0, 1, 1] == 0).all()) and bool((idx[0, 0, 0] == 8).all())
    x[0, 1, 2, 1::2] = float("nan")                   # a second NaN, after the first in windows (0, 1) and (1, 1)
    x[0, 0, 1, 0::2] = float("nan")                   # and one before it in windows (0, 0) and (0, 1)
    x[1, 6, 8, :] = float("nan")                      # the last pixel of the last image
    y2, idx2 = _check_fwd(nb, x, k, s, p, dtype, what="two NaNs")
    assert torch.equal(idx2[0, 1, 1], idx[0, 1, 1])   # the first NaN stays
    assert bool((idx2[0, 0, 0, 0::2] == 1 * k + 2).all()) and bool((idx2[0, 0, 0, 1::2] == 8).all())

    x = _fill("randn", (N, H, W, C), g)
    x[0, :2, :2, :] = float("-inf")                   # the window (0, 0) of image 0 sees nothing else
    y, idx = _check_fwd(nb, x, k, s, p, dtype, what="-inf window")
    assert bool((idx[0, 0, 0] == 1 * k + 1).all()) and bool((y[0, 0, 0] == float("-inf")).all())
    OH, OW = _osz(H, W, k, s, p)
    dy = _fill("dyadic", (N, OH, OW, C), g, zeros=0).to(dtype)
    dx = _out(N * H * W, C, C, 0, dtype)
    nb.C.maxpool_bwd(dy.view(-1, C), idx.reshape(-1), N, H, W, C, k, s, p, OH, OW, None, 0, 0, dx, C, 0)
    ref = R.maxpool_bwd(dy, idx, H, W, k, s, p)        # asserts that every index names an in-image tap
    assert torch.equal(dx.view(N, H, W, C).double(), ref)   # dyadic: every sum is exact
    assert torch.equal(dx.view(N, H, W, C)[0, 0, 0], dy[0, 0, 0])


# ------------------------------------------------------------------ max pool backward
def _nwin(k, s):
    return math.ceil(k / s)


def _check_bwd(nb, dy, idx, H, W, k, s, p, add, ldadd, addoff, lddx, dxoff, what):
    """The plain backward: dx (a slice of a sentinel slab) against the scatter by the kernel's idx."""
    N, OH, OW, C = dy.shape
    dtype = dy.dtype
    addbuf = None if add is None else _slab(add, ldadd, addoff, dtype)
    dxbuf = _out(N * H * W, C, lddx, dxoff, dtype)
    nb.C.maxpool_bwd(dy.view(-1, C), idx.reshape(-1), N, H, W, C, k, s, p, OH, OW, addbuf, ldadd, addoff, dxbuf, lddx,
                     dxoff)
    dx = _cut(dxbuf, dxoff, C, (N, H, W))
    adds = None if add is None else _cut(addbuf, addoff, C, (N, H, W))
    ref, mag = R.maxpool_bwd_terms(dy, idx, H, W, k, s, p, adds)
    n = _nwin(k, s) ** 2 + (add is not None)
    err, tol = (dx.double() - ref).abs(), R.store_tol(ref, dtype) + n * U * mag
    assert _le(err, tol), f"{what}: {_worst(err, tol)}"
    assert _outside_untouched(dxbuf, dxoff, C), f"{what}: dx wrote outside its slice"
    if add is not None:
        assert _outside_untouched(addbuf, addoff, C)
    if k == 2 and s == 2 and p == 0:   # floor mode: the last odd row / column is in no window
        base = torch.zeros_like(dx) if add is None else adds
        if H % 2:
            assert torch.equal(dx[:, H - 1], base[:, H - 1]), f"{what}: uncovered row"
        if W % 2:
            assert torch.equal(dx[:, :, W - 1], base[:, :, W - 1]), f"{what}: uncovered column"
    return dx


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GEOMS, ids=_id)
def test_maxpool_bwd(nb, case, dtype, fill):
    """Every geometry, fed the kernel's own idx: without add, with add as the slice ld 192 / off 128, and
    (C <= 56) with dx as the slice ld 64 / off 8."""
    k, s, p, N, H, W, C = case
    g = _gen(*case, fill, "bwd")
    _, idx = _mp_fwd(nb, _slab(_fill(fill, (N, H, W, C), g), C, 0, dtype), N, H, W, C, C, 0, k, s, p)
    OH, OW = _osz(H, W, k, s, p)
    dy = _fill(fill, (N, OH, OW, C), g, zeros=0.1).to(dtype)
    add = _fill(fill, (N, H, W, C), g, zeros=0.1)
    ldadd, addoff = (192, 128) if C <= 64 else (C + 64, 64)
    _check_bwd(nb, dy, idx, H, W, k, s, p, None, 0, 0, C, 0, "no add")
    _check_bwd(nb, dy, idx, H, W, k, s, p, add, ldadd, addoff, C, 0, "add slice")
    if C <= 56:
        _check_bwd(nb, dy, idx, H, W, k, s, p, add, C, 0, 64, 8, "dx slice")
        _check_bwd(nb, dy, idx, H, W, k, s, p, None, 0, 0, 64, 8, "dx slice, no add")


def _fused_blocks(M, C):
    rpb = 256 // (C // 8)
    return max(1, min(4096, math.ceil(M / (rpb * 8))))


def chain_len(M, C, nblk):
    """L: the longest fp32 chain of a row reduction -- the rows one lane walks, then the RPB lanes."""
    rpb = 256 // (C // 8)
    return math.ceil(M / (nblk * rpb)) + rpb


def _check_partials(part, M, C, dx, z, what):
    """part [nblk][2][C] against the sums of the STORED dx: (L + r) u sum|term|, r = 1 (sum dx), 2 (sum dx z)."""
    nblk = _fused_blocks(M, C)
    assert tuple(part.shape) == (nblk, 2, C)
    L = chain_len(M, C, nblk)
    ref, mag = R.masked_sums(dx.reshape(M, C), z.reshape(M, C))
    got = part.double().sum(0)
    for row, r in ((0, 1), (1, 2)):
        err, tol = (got[row] - ref[row]).abs(), (L + r) * U * mag[row]
        assert _le(err, tol), f"{what} partial row {row}: {_worst(err, tol)}"


# C = 2048: one row lane per block (RPB = 1); M = 257 (C = 24: RPB = 85, four blocks); (2,7,9,8): M = 126, less
# than the 256 row lanes of its single block; C = 24 / 40: 256 % (C/8) != 0, inactive lanes
FUSED_EXTRA = [(3, 2, 1, 1, 4, 4, 2048), (3, 2, 1, 1, 257, 1, 24), (2, 2, 0, 2, 8, 6, 24), (2, 2, 0, 1, 257, 2, 8)]


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GEOMS + FUSED_EXTRA, ids=_id)
def test_maxpool_bwd_fused(nb, case, dtype, with_add):
    """maxpool_bwd_bn (NWIN 1, 2 and the general loop): dx exactly the masked plain result, the mask
    exact, the partials of the stored dx."""
    k, s, p, N, H, W, C = case
    g = _gen(*case, "fused")
    M = N * H * W
    z = _slab(_dyadic((N, H, W, C), g), C, 0, dtype)
    sc, sh = _bn_coef(C, g)
    _, idx = _mp_fwd(nb, z, N, H, W, C, C, 0, k, s, p, bn=(sc, sh))
    OH, OW = _osz(H, W, k, s, p)
    dy = _dyadic((N, OH, OW, C), g, zeros=0.1).to(dtype)
    ldadd, addoff = (192, 128) if C <= 64 else (C + 64, 64)
    addbuf = _slab(_dyadic((N, H, W, C), g, zeros=0.1), ldadd, addoff, dtype) if with_add else None
    dx = _out(M, C, C, 0, dtype)
    part = nb.C.maxpool_bwd_bn(dy.view(-1, C), idx.reshape(-1), N, H, W, C, k, s, p, OH, OW, z, sc, sh, addbuf,
                               ldadd if with_add else 0, addoff if with_add else 0, dx)
    plain = _out(M, C, C, 0, dtype)
    nb.C.maxpool_bwd(dy.view(-1, C), idx.reshape(-1), N, H, W, C, k, s, p, OH, OW, addbuf,
                     ldadd if with_add else 0, addoff if with_add else 0, plain, C, 0)
    mask = R.relu_mask(z, sc, sh)
    if M * C >= 512:   # the fill reaches every kind of mask decision, exact zeros (masked out) included
        assert 0 < int(mask.sum()) < mask.numel() and bool(((z.double() * sc.double() + sh.double()) == 0).any())
    assert torch.equal(dx, torch.where(mask, plain, torch.zeros_like(plain))), "dx is not the masked plain result"
    adds = _cut(addbuf, addoff, C, (N, H, W)) if with_add else None
    ref, mag = R.maxpool_bwd_terms(dy, idx, H, W, k, s, p, adds)
    ref = torch.where(mask.view(N, H, W, C), ref, torch.zeros_like(ref))
    n = _nwin(k, s) ** 2 + with_add
    err, tol = (dx.view(N, H, W, C).double() - ref).abs(), R.store_tol(ref, dtype) + n * U * mag
    assert _le(err, tol), f"dx: {_worst(err, tol)}"
    _check_partials(part, M, C, dx, z, _id(case))
    if with_add:
        assert _outside_untouched(addbuf, addoff, C)


# ------------------------------------------------------------------ outer_dgrad_bn / head_dgrad_bn
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 257, 1000])
@pytest.mark.parametrize("C", [8, 24, 64, 2048])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_head_dgrad(nb, K, C, M, dtype):
    """dx = mask * dl w^T from rows of 8 (lddl = ldw = 8) whose padding columns are NaN; K = 1 is
    outer_dgrad_bn."""
    for fill in FILLS:
        g = _gen(K, C, M, fill)
        dl = torch.full((M, 8), float("nan"), device=DEV, dtype=dtype)
        w = torch.full((C, 8), float("nan"), device=DEV, dtype=dtype)
        dl[:, :K] = _fill(fill, (M, K), g, zeros=0.1).to(dtype)
        w[:, :K] = _fill(fill, (C, K), g, zeros=0.1).to(dtype)
        z = _dyadic((M, C), g).to(dtype)
        sc, sh = _bn_coef(C, g)
        dx = _out(M, C, C, 0, dtype)
        if K == 1:
            part = nb.C.outer_dgrad_bn(dl, 8, M, C, w, 8, z, sc, sh, dx)
        else:
            part = nb.C.head_dgrad_bn(dl, 8, K, M, C, w, 8, z, sc, sh, dx)
        ref, mag = R.head_dgrad_terms(dl[:, :K], w[:, :K], z, sc, sh)
        err, tol = (dx.double() - ref).abs(), R.store_tol(ref, dtype) + K * U * mag
        assert _le(err, tol), f"{fill} dx: {_worst(err, tol)}"
        mask = R.relu_mask(z, sc, sh)
        assert bool((dx[~mask] == 0).all()), f"{fill}: a masked-out element is not zero"
        if fill == "dyadic":   # products and sums exact in fp32: the stored dx is the rounded reference
            assert torch.equal(dx.double(), ref.to(dtype).double())
        _check_partials(part, M, C, dx, z, f"{fill} K={K}")


# ------------------------------------------------------------------ global average pool
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C", [8, 24, 512])
@pytest.mark.parametrize("HW", [1, 2, 49, 50])
def test_avgpool(nb, HW, C, N, dtype):
    for fill in FILLS:
        g = _gen(HW, C, N, fill)
        x = _fill(fill, (N, HW, C), g).to(dtype)
        y = _out(N, C, C, 0, dtype)
        nb.C.avgpool_fwd(x.view(-1, C), N, HW, C, y)
        ref, mag = R.avgpool_terms(x)
        err, tol = (y.double() - ref).abs(), R.store_tol(ref, dtype) + (HW + 2) * U * mag
        assert _le(err, tol), f"{fill} forward: {_worst(err, tol)}"
        dy = _fill(fill, (N, C), g, zeros=0.1).to(dtype)
        dx = _out(N * HW, C, C, 0, dtype)
        nb.C.avgpool_bwd(dy, N, HW, C, dx)
        ref = R.avgpool_bwd(dy, HW)
        err, tol = (dx.view(N, HW, C).double() - ref).abs(), R.store_tol(ref, dtype) + 2 * U * ref.abs()
        assert _le(err, tol), f"{fill} backward: {_worst(err, tol)}"


# ------------------------------------------------------------------ bilinear x2
UP_SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (16, 16), (33, 17), (257, 2), (2, 300)]
UP_CASES = [(H, W, C) for (H, W) in UP_SIZES for C in (8, 24)] + [(16, 16, 64)]


def _coord(H, W):
    """The coordinate term's factor: o * fl((n-1)/(2n-1)) lies within dn = 2u (n-1) of the exact coordinate
    on each axis; a bilinear interpolant moves by at most (dH + dW + dH dW) times the footprint's |x|."""
    dh, dw = 2 * U * (H - 1), 2 * U * (W - 1)
    return dh + dw + dh * dw


def _up_fwd(nb, x, ldx, xoff, ldy, yoff):
    N, H, W, C = x.shape
    xbuf = _slab(x, ldx, xoff, x.dtype)
    ybuf = _out(N * 4 * H * W, C, ldy, yoff, x.dtype)
    nb.C.upsample2x_fwd(xbuf, N, H, W, C, ldx, xoff, ybuf, ldy, yoff)
    assert _outside_untouched(ybuf, yoff, C) and _outside_untouched(xbuf, xoff, C)
    return _cut(ybuf, yoff, C, (N, 2 * H, 2 * W))


def _up_fwd_tol(x):
    ref = R.upsample(x)
    mag, foot = R.upsample_terms(x)
    return ref, R.store_tol(ref, x.dtype) + 6 * U * mag + _coord(x.shape[1], x.shape[2]) * foot


def _up_bwd(nb, gy, lddy, dyoff):
    N, OH, OW, C = gy.shape
    gbuf = _slab(gy, lddy, dyoff, gy.dtype)
    dx = _out(N * OH * OW // 4, C, C, 0, gy.dtype)
    nb.C.upsample2x_bwd(gbuf, N, OH // 2, OW // 2, C, lddy, dyoff, dx)
    assert _outside_untouched(gbuf, dyoff, C)
    return dx.view(N, OH // 2, OW // 2, C)


def _up_bwd_tol(gy):
    ref = R.upsample_bwd(gy)
    mag, foot, count = R.upsample_bwd_terms(gy)
    return ref, R.store_tol(ref, gy.dtype) + (6 + count) * U * mag + _coord(ref.shape[1], ref.shape[2]) * foot


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,C", UP_CASES)
def test_bilinear(nb, H, W, C, dtype):
    """Forward and backward elementwise, dense and (C <= 56) as the UNet concat's slices: x ld 64 / off 8,
    y and dy ld 192 / off 128."""
    N = 2
    for fill in FILLS:
        g = _gen(H, W, C, fill)
        x = _fill(fill, (N, H, W, C), g, zeros=0.1).to(dtype)
        gy = _fill(fill, (N, 2 * H, 2 * W, C), g, zeros=0.1).to(dtype)
        ref, tol = _up_fwd_tol(x)
        bref, btol = _up_bwd_tol(gy)
        for sliced in ([False, True] if C <= 56 else [False]):
            y = _up_fwd(nb, x, *((64, 8, 192, 128) if sliced else (C, 0, C, 0)))
            err = (y.double() - ref).abs()
            assert _le(err, tol), f"{fill} forward sliced={sliced}: {_worst(err, tol)}"
            dx = _up_bwd(nb, gy, *((192, 128) if sliced else (C, 0)))
            err = (dx.double() - bref).abs()
            assert _le(err, btol), f"{fill} backward sliced={sliced}: {_worst(err, btol)}"


@pytest.mark.parametrize("H,W", [(3, 7), (33, 17), (2, 300)])
def test_bilinear_adjoint(nb, H, W):
    """<up(x), g> == <x, up_bwd(g)> in fp32 storage, sums in fp64, within the two bounds combined
    (secondary to the fp64 comparisons: both sides are kernels)."""
    g = _gen(H, W, "adjoint")
    x = torch.randn(2, H, W, 8, generator=g, device=DEV)
    gy = torch.randn(2, 2 * H, 2 * W, 8, generator=g, device=DEV)
    y, dx = _up_fwd(nb, x, 8, 0, 8, 0), _up_bwd(nb, gy, 8, 0)
    lhs, rhs = (y.double() * gy.double()).sum(), (x.double() * dx.double()).sum()
    tol = (_up_fwd_tol(x)[1] * gy.double().abs()).sum() + (_up_bwd_tol(gy)[1] * x.double().abs()).sum()
    assert abs(lhs.item() - rhs.item()) <= tol.item(), (lhs.item(), rhs.item(), tol.item())


# ------------------------------------------------------------------ layouts (exact)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,Cpad", [(1, 8), (3, 8), (4, 8), (8, 8), (9, 16)])
def test_nchw_to_nhwc(nb, C, Cpad, dtype):
    N, H, W = 2, 5, 7
    x = torch.randn(N, C, H, W, generator=_gen(C, Cpad), device=DEV)
    y = _out(N * H * W, Cpad, Cpad, 0, dtype)
    nb.C.nchw_to_nhwc(x, N, C, H, W, Cpad, y)
    assert _bits_equal(y, R.nchw_to_nhwc_pad(x, Cpad, F32).view(-1, Cpad))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,CS", [(3, 4), (1, 2)])
@pytest.mark.parametrize("H,W,pad", [(5, 7, 3), (8, 8, 1), (1, 1, 3), (23, 17, 3)])
def test_s2d(nb, H, W, pad, C, CS, dtype):
    N = 2
    Us, V = (H + 2 * pad + 1) // 2, (W + 2 * pad + 1) // 2
    x = torch.randn(N, C, H, W, generator=_gen(H, W, pad, C), device=DEV)
    y = _out(N * Us * V, 4 * CS, 4 * CS, 0, dtype)
    nb.C.s2d_nchw(x, N, C, H, W, pad, Us, V, CS, y)
    assert _bits_equal(y, R.s2d(x, pad, Us, V, CS, F32).view(-1, 4 * CS))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("Kp", [8, 16])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8])
def test_nhwc_pad_cast(nb, K, Kp, M, dtype):
    x = torch.randn(M, K, generator=_gen(K, Kp, M), device=DEV)
    y = _out(M, Kp, Kp, 0, dtype)
    nb.C.nhwc_pad_cast(x, M, K, Kp, y)
    assert _bits_equal(y, R.pad_cast(x, Kp, F32))


# ------------------------------------------------------------------ the second trip of the capped grids
TRIP = 16384 * 256 + 256   # threads: one block more than the 16384-block cap holds
TH, TW = 1856, 2260        # TH * TW == TRIP


def test_second_trip_maxpool(nb):
    """maxpool_fwd_fixed (2x2/s2), maxpool_fwd (runtime 2x2/s1) and maxpool_bwd past the grid cap, bf16,
    the whole output against the reference in the storage type (selection and single additions: exact)."""
    assert TH * TW == TRIP
    g = _gen("trip", "maxpool")
    C = 8
    x = _dyadic((1, TH + 1, TW + 1, C), g).to(BF16)
    y, idx = _mp_fwd(nb, x.view(-1, C), 1, TH + 1, TW + 1, C, C, 0, 2, 1, 0)       # TH x TW outputs
    yr, ir = R.maxpool(x, 2, 1, 0, dtype=BF16)
    assert torch.equal(y, yr) and torch.equal(idx, ir)
    del y, idx, yr, ir
    x = _dyadic((1, 2 * TH, 2 * TW, C), g).to(BF16)
    y, idx = _mp_fwd(nb, x.view(-1, C), 1, 2 * TH, 2 * TW, C, C, 0, 2, 2, 0)
    yr, ir = R.maxpool(x, 2, 2, 0, dtype=BF16)
    assert torch.equal(y, yr) and torch.equal(idx, ir)
    del x, y, yr, ir, idx
    # backward: TH x TW input pixels; one window per pixel, so dx = dy (or 0) + add is one bf16-exact sum
    H, W = TH, TW
    x = _dyadic((1, H, W, C), g).to(BF16)
    _, idx = _mp_fwd(nb, x.view(-1, C), 1, H, W, C, C, 0, 2, 2, 0)
    dy = _dyadic((1, H // 2, W // 2, C), g, zeros=0.1).to(BF16)
    add = _dyadic((1, H, W, C), g, zeros=0.1).to(BF16)
    dx = _out(H * W, C, C, 0, BF16)
    nb.C.maxpool_bwd(dy.view(-1, C), idx.reshape(-1), 1, H, W, C, 2, 2, 0, H // 2, W // 2, add.view(-1, C), C, 0, dx,
                     C, 0)
    ref = R.maxpool_bwd(dy, idx, H, W, 2, 2, 0, add, dtype=F32)   # multiples of 1/8 up to 8: exact in bf16
    assert torch.equal(dx.view(1, H, W, C).float(), ref)


def test_second_trip_avgpool(nb):
    N, HW, C = TRIP // 8, 2, 64          # forward: N * C/8 threads
    x = _dyadic((N, HW, C), _gen("trip", "avg")).to(BF16)
    y = _out(N, C, C, 0, BF16)
    nb.C.avgpool_fwd(x.view(-1, C), N, HW, C, y)
    ref, mag = R.avgpool_terms(x)
    err, tol = (y.double() - ref).abs(), R.store_tol(ref, BF16) + (HW + 2) * U * mag
    assert _le(err, tol), _worst(err, tol)
    del x, y, ref, mag, err, tol
    N, HW, C = TH, TW, 8                 # backward: N * HW * C/8 threads
    assert N * HW == TRIP
    dy = _dyadic((N, C), _gen("trip", "avgb"), zeros=0.1).to(BF16)
    dx = _out(N * HW, C, C, 0, BF16)
    nb.C.avgpool_bwd(dy, N, HW, C, dx)
    ref = R.avgpool_bwd(dy, HW)
    err, tol = (dx.view(N, HW, C).double() - ref).abs(), R.store_tol(ref, BF16) + 2 * U * ref.abs()
    assert _le(err, tol), _worst(err, tol)


def test_second_trip_layouts(nb):
    g = _gen("trip", "layout")
    x = torch.randn(1, 3, TH, TW, generator=g, device=DEV)            # TH * TW pixels x Cpad / 8 = 1
    y = _out(TH * TW, 8, 8, 0, BF16)
    nb.C.nchw_to_nhwc(x, 1, 3, TH, TW, 8, y)
    assert _bits_equal(y, R.nchw_to_nhwc_pad(x, 8, F32).view(-1, 8))
    del x, y
    pad, Us, V = 3, TH, TW // 2                                       # U * V pixels x (4 CS / 8 = 2)
    H, W = 2 * Us - 2 * pad - 1, 2 * V - 2 * pad
    assert (H + 2 * pad + 1) // 2 == Us and (W + 2 * pad + 1) // 2 == V and Us * V * 2 == TRIP
    x = torch.randn(1, 3, H, W, generator=g, device=DEV)
    y = _out(Us * V, 16, 16, 0, BF16)
    nb.C.s2d_nchw(x, 1, 3, H, W, pad, Us, V, 4, y)
    assert _bits_equal(y, R.s2d(x, pad, Us, V, 4, F32).view(-1, 16))
    del x, y
    M, K, Kp = TRIP, 3, 8                                             # nhwc_pad_cast: M * Kp / 8 threads
    x = torch.randn(M, K, generator=g, device=DEV)
    y = _out(M, Kp, Kp, 0, BF16)
    nb.C.nhwc_pad_cast(x, M, K, Kp, y)
    assert _bits_equal(y, R.pad_cast(x, Kp, F32))


def test_second_trip_bilinear(nb):
    """N * 4HW * C/8 = TRIP forward threads (H, W = 116, 113), N * HW * C/8 backward (232, 226): the sizes
    stay below 300, where the float coordinate's floor is the exact one."""
    g = _gen("trip", "bilinear")
    N, H, W, C = 5, 116, 113, 128
    assert N * 4 * H * W * (C // 8) == TRIP
    x = torch.randn(N, H, W, C, generator=g, device=DEV).to(BF16)
    y = _up_fwd(nb, x, C, 0, C, 0)
    ref, tol = _up_fwd_tol(x)
    err = (y.double() - ref).abs()
    assert _le(err, tol), _worst(err, tol)
    del x, y, ref, tol, err
    N, H, W, C = 5, 232, 226, 128
    assert N * H * W * (C // 8) == TRIP
    gy = torch.randn(N, 2 * H, 2 * W, C, generator=g, device=DEV).to(BF16)
    dx = _up_bwd(nb, gy, C, 0)
    ref, tol = _up_bwd_tol(gy)
    err = (dx.double() - ref).abs()
    assert _le(err, tol), _worst(err, tol)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(nb, dtype):
    """Nothing launches and the outputs keep their sentinels: C % 8 in the three launchers that had no
    check, a window an index byte cannot describe (k = 17), a window wholly in padding (2 pad > k)."""
    N, H, W, C = 1, 4, 4, 12
    x = torch.ones(N * H * W, C, device=DEV, dtype=dtype)
    y = _out(N, C, C, 0, dtype)
    with pytest.raises(RuntimeError, match="avgpool_fwd"):
        nb.C.avgpool_fwd(x, N, H * W, C, y)
    assert bool((y == SENT).all())
    dx = _out(N * H * W, C, C, 0, dtype)
    with pytest.raises(RuntimeError, match="avgpool_bwd"):
        nb.C.avgpool_bwd(torch.ones(N, C, device=DEV, dtype=dtype), N, H * W, C, dx)
    assert bool((dx == SENT).all())
    up = _out(N * 4 * H * W, C, C, 0, dtype)
    with pytest.raises(RuntimeError, match="upsample2x_fwd"):
        nb.C.upsample2x_fwd(x, N, H, W, C, C, 0, up, C, 0)
    assert bool((up == SENT).all())
    for (k, s, p, HH) in [(17, 2, 8, 20), (3, 2, 2, 6), (2, 2, 2, 6), (0, 2, 0, 6), (3, 0, 1, 6), (3, 2, -1, 6)]:
        C = 8
        OH = R.out_size(HH, k, s, p) if s > 0 else 1
        xb = torch.ones(HH * HH, C, device=DEV, dtype=dtype)
        yb = _out(OH * OH, C, C, 0, dtype)
        idx = torch.full((OH * OH * C,), ISENT, dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match="maxpool_fwd"):
            nb.C.maxpool_fwd(xb, 1, HH, HH, C, C, 0, k, s, p, yb, idx, OH, OH, None, None, None, 0, 0)
        assert bool((yb == SENT).all()) and bool((idx == ISENT).all()), (k, s, p)
