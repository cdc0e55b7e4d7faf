"""The BatchNorm kernel family (csrc/kernels/bn.hip, bnfin.h) against the fp64 reference of
tests/bn_ref.py at its edge shapes: every row map, channel slices, both trips of the grid-stride
loops, every column-reduce path with odd channel counts, the backward finalize, the argument checks.

Every stage is compared with fp64 computed on the device from the SAME stored inputs, the kernel's
own fp32 outputs of the stage before included, so a bound is the error of one kernel.  Comparisons
are elementwise (per channel for the sums) and the bounds count roundings (profiles/bn_tests/README.md
derives each k and L); u = 2^-24:

* elementwise kernels  |out - ref| <= h(ref) + k u mag, mag = the sum of the absolute terms, h = half a
  bf16 ulp of ref (0 for fp32 storage); mask bits and dyr_out exact;
* row reductions       |sum_k partial[k] - ref| <= (L + r) u sum|term| per channel;
* finalize kernels     k u relative per output (shift, running statistics, dgamma / dbeta: k u times
  the sum of the absolute terms), with the k written next to each line of bnfin.h.
"""
import math

import pytest
import torch

import bn_ref as R
from deeplearning_mpi_amd.ops.act import Act, Deferred
from deeplearning_mpi_amd.ops.backend import NativeBackend

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
EPS = 1e-5
SENT = 640.0   # exact in bf16; no kernel output below comes near it


@pytest.fixture(scope="module")
def nb():
    return NativeBackend(DEV)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _f32(v):
    """The value a float argument has once the binding has cast it to fp32."""
    return torch.tensor(v, dtype=F32).item()


def _mu(C, g):
    """Per-channel offsets of random sign with |mu| in [1, 2)."""
    sign = torch.randint(0, 2, (C,), generator=g, device=DEV).float() * 2 - 1
    return sign * (1 + torch.rand(C, generator=g, device=DEV))


def _sliced(M, C, ld, off, dtype, g, mu=None, fill=None):
    """An [M, ld] buffer of the storage type and its channel slice [off, off + C)."""
    assert ld % 8 == 0 and off % 8 == 0 and off + C <= ld
    if fill is not None:
        buf = torch.full((M, ld), fill, device=DEV, dtype=dtype)
    else:
        buf = torch.randn(M, ld, generator=g, device=DEV)
        if mu is not None:
            buf[:, off:off + C] += mu
        buf = buf.to(dtype)
    return buf, buf[:, off:off + C]


def _relu_like(M, C, ld, off, dtype, g):
    """A stored ReLU output: positive, exactly zero and (as a mask only) negative values."""
    buf = torch.randn(M, ld, generator=g, device=DEV)
    buf[torch.rand(M, ld, generator=g, device=DEV) < 0.4] = 0.0
    buf = buf.to(dtype)
    return buf, buf[:, off:off + C]


def _outside_untouched(buf, off, C, fill=SENT):
    keep = torch.ones(buf.shape[1], dtype=torch.bool, device=buf.device)
    keep[off:off + C] = False
    return bool((buf[:, keep] == fill).all())


def _le(err, tol):
    """err <= tol everywhere (a NaN on either side fails)."""
    return bool((err <= tol).all())


def _worst(err, tol):
    r = torch.nan_to_num(err / tol.clamp_min(1e-300), nan=float("inf"))
    return f"worst err / bound = {r.max().item():.3g} at {tuple(int(i) for i in (r == r.max()).nonzero()[0])}"


# ------------------------------------------------------------------ stage checks
def chain_len(M, C, nblk):
    """L: the longest fp32 chain of a row reduction -- the rows one lane walks, then the RPB lanes."""
    rpb = 256 // (C // 8)
    return math.ceil(M / (nblk * rpb)) + rpb


def check_sums(part, nblk, ref, absref, L, r, what):
    """part [>= nblk][2][C] fp32 block partials against per-channel fp64 sums ref [2][C]."""
    got = part[:nblk].double().sum(0)
    for k in range(2):
        if ref[k] is None:
            continue
        err, tol = (got[k] - ref[k]).abs(), (L + r[k]) * U * absref[k]
        assert _le(err, tol), f"{what} row {k}: {_worst(err, tol)}"


def check_apply(x, scale, shift, res, rscale, rshift, relu, y, bits, what):
    """y, bits: the kernel's stored output slice and mask bytes; the operands as the kernel read them."""
    pre, mag = R.apply_terms(x, scale, shift, res, rscale, rshift)
    ref = pre.clamp_min(0.0) if relu else pre
    k = 1 + (res is not None) + (rscale is not None)   # the fma, the residual's fma, the sum
    err, tol = (y.double() - ref).abs(), R.store_tol(ref, y.dtype) + k * U * mag
    assert _le(err, tol), f"{what}: {_worst(err, tol)}"
    if bits is not None:
        assert torch.equal(bits, R.mask_bits(y)), f"{what}: mask bits != stored y > 0"


def check_bwd_apply(dy, ymask, x, coef, dx, dyr_out, what):
    dyr = R.masked(dy, ymask)
    ref, mag = R.bwd_apply_terms(dyr, x, coef[0], coef[1], coef[2])
    err, tol = (dx.double() - ref).abs(), R.store_tol(ref, dx.dtype) + 2 * U * mag   # two fmas
    assert _le(err, tol), f"{what} dx: {_worst(err, tol)}"
    if dyr_out is not None:
        assert torch.equal(dyr_out.double(), dyr), f"{what}: dyr_out is not the masked dy"


def check_fwd_finalize(st, T, count, gamma, beta, rm0, rv0, mom, out, rm, rv, what):
    """out [4][C] = scale, shift, mean, invstd from the kernel; st [T][2][C] the partials it read."""
    s = st[:T].double().sum(0)
    f = R.fwd_finalize(s[0], s[1], count, gamma, beta, _f32(EPS), rm0, rv0, _f32(mom))
    beta_abs = 0.0 if beta is None else beta.double().abs()
    rows = [("scale", out[0], f["scale"], 3 * U * f["scale"].abs()),
            ("shift", out[1], f["shift"], 6 * U * (beta_abs + (f["mean"] * f["scale"]).abs())),
            ("mean", out[2], f["mean"], 2 * U * f["mean"].abs()),
            ("invstd", out[3], f["invstd"], 2 * U * f["invstd"].abs())]
    if rm0 is not None:
        rows += [("running_mean", rm, f["running_mean"], 6 * U * (rm0.double().abs() + f["mean"].abs())),
                 ("running_var", rv, f["running_var"], 6 * U * (rv0.double().abs() + f["unbiased"].abs()))]
    for name, got, ref, tol in rows:
        assert bool(torch.isfinite(got).all()), f"{what} {name}: not finite"
        err = (got.double() - ref).abs()
        assert _le(err, tol), f"{what} {name}: {_worst(err, tol)}"
    return f


def check_bwd_finalize(part, T, k2, raw_z, count, gamma, mean, invstd, dg0, db0, dg, db, coef, what):
    s1, s2 = part[:T, 0].double().sum(0), part[:T, k2].double().sum(0)
    if raw_z:
        s2 = R.raw_to_xhat(s1, s2, mean, invstd)
    if coef is not None:
        k = R.bwd_finalize(s1, s2, count, gamma, mean, invstd)
        for i, name in enumerate(("k1", "k2", "k3")):
            err, tol = (coef[i].double() - k[name]).abs(), 2 * U * k[name].abs()
            assert _le(err, tol), f"{what} {name}: {_worst(err, tol)}"
    for name, got, old, s in (("dgamma", dg, dg0, s2), ("dbeta", db, db0, s1)):
        if got is None:
            continue
        err, tol = (got.double() - (old.double() + s)).abs(), 3 * U * (old.double().abs() + s.abs())
        assert _le(err, tol), f"{what} {name}: {_worst(err, tol)}"


# ------------------------------------------------------------------ A. row maps
def _rpb(C):
    return 256 // (C // 8)


ROWMAP_CASES = [(C, M) for C in (8, 24, 72, 192, 264, 2048) for M in (1, _rpb(C) + 1, 33 * _rpb(C) + 3)]
ROWMAP_CASES.append((2048, 16384 + 5))   # reduce_blocks caps the grid at 1024 blocks


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,M", ROWMAP_CASES)
def test_row_reductions(nb, C, M, dtype):
    """bn_stats, bn_bwd_reduce (with and without ymask) and channel_sum at every row map."""
    g = _gen(C * 131 + M)
    nblk = nb.C.reduce_blocks(M, C)
    assert nblk == min(1024, max(1, math.ceil(M / (16 * _rpb(C)))))
    L = chain_len(M, C, nblk)
    _, x = _sliced(M, C, C, 0, dtype, g, _mu(C, g))
    _, dy = _sliced(M, C, C, 0, dtype, g, _mu(C, g))
    _, ym = _relu_like(M, C, C, 0, dtype, g)
    xd = x.double()
    mean = (xd.mean(0) + 0.1 * torch.randn(C, generator=g, device=DEV).double()).float()
    invstd = torch.rand(C, generator=g, device=DEV) + 0.5

    def partial():   # one row more than the launch writes: it must stay as it is
        return torch.full((nblk + 1, 2, C), float("nan"), device=DEV)

    part = partial()
    nb.C.bn_stats(x, M, C, C, 0, part, nblk)
    check_sums(part, nblk, R.sums(x), (xd.abs().sum(0), (xd * xd).sum(0)), L, (1, 2), "bn_stats")
    assert bool(part[nblk].isnan().all())

    xhat = (xd - mean.double()) * invstd.double()
    for mask in (None, ym):
        dyr = R.masked(dy, mask)
        part = partial()
        nb.C.bn_bwd_reduce(dy, C, 0, mask, C, 0, x, C, 0, M, C, mean, invstd, part, nblk)
        check_sums(part, nblk, R.bwd_reduce(dy, mask, x, mean, invstd),
                   (dyr.abs().sum(0), (dyr * xhat).abs().sum(0)), L, (1, 4),
                   f"bn_bwd_reduce mask={mask is not None}")
        assert bool(part[nblk].isnan().all())
    # the x == null form sums dyr alone (row 1 stays zero)
    part = partial()
    nb.C.bn_bwd_reduce(dy, C, 0, ym, C, 0, None, 0, 0, M, C, None, None, part, nblk)
    dyr = R.masked(dy, ym)
    check_sums(part, nblk, (dyr.sum(0), torch.zeros(C, device=DEV, dtype=F64)),
               (dyr.abs().sum(0), torch.zeros(C, device=DEV, dtype=F64)), L, (1, 0), "bn_bwd_reduce x=None")

    # channel_sum: the same reduction, finalized into out_acc += sum (the cast and the sum: 2 more)
    acc0 = torch.randn(C, generator=g, device=DEV) * 3
    acc = acc0.clone()
    nb.C.channel_sum(x, M, C, C, 0, acc)
    ref = acc0.double() + xd.sum(0)
    err, tol = (acc.double() - ref).abs(), (L + 1 + 2) * U * (xd.abs().sum(0) + acc0.double().abs())
    assert _le(err, tol), f"channel_sum: {_worst(err, tol)}"


# ------------------------------------------------------------------ B. slices
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [24, 192])
def test_sliced_operands(nb, C, dtype):
    """Every operand in a wider buffer of its own, each with another ld and a non-zero offset; the
    outputs land in their slice and nowhere else."""
    g = _gen(C)
    M = 1403   # 2 blocks at C = 24, 9 at C = 192
    xb, x = _sliced(M, C, C + 8, 8, dtype, g, _mu(C, g))
    rb_, res = _sliced(M, C, C + 16, 16, dtype, g)
    yb, y = _sliced(M, C, 2 * C, C - 8, dtype, g, fill=SENT)
    dyb, dy = _sliced(M, C, C + 40, 8, dtype, g, _mu(C, g))
    ymb, ym = _sliced(M, C, 2 * C + 8, C, dtype, g, fill=SENT)
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    nblk = nb.C.reduce_blocks(M, C)
    L = chain_len(M, C, nblk)
    xd = x.double()

    part = torch.empty(nblk, 2, C, device=DEV)
    nb.C.bn_stats(xb, M, C, C + 8, 8, part, nblk)
    check_sums(part, nblk, R.sums(x), (xd.abs().sum(0), (xd * xd).sum(0)), L, (1, 2), "bn_stats")
    v = torch.empty(4, C, device=DEV)
    rm0, rv0 = torch.randn(C, generator=g, device=DEV), torch.rand(C, generator=g, device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    nb.C.bn_finalize(part, nblk, C, float(M), gamma, beta, rm, rv, 0.1, EPS, v[0], v[1], v[2], v[3])
    check_fwd_finalize(part, nblk, M, gamma, beta, rm0, rv0, 0.1, v, rm, rv, "bn_finalize")

    bits = torch.full((M, C // 8), 0xA5, dtype=torch.uint8, device=DEV)
    nb.C.bn_apply(xb, C + 8, 8, M, C, v[0], v[1], rb_, C + 16, 16, True, yb, 2 * C, C - 8, bits, None, None)
    check_apply(x, v[0], v[1], res, None, None, True, y, bits, "bn_apply")
    assert _outside_untouched(yb, C - 8, C), "bn_apply wrote outside its y slice"
    # the Deferred.bn residual through the same slices
    rs, rh = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    y2b, y2 = _sliced(M, C, C + 32, 24, dtype, g, fill=SENT)
    nb.C.bn_apply(xb, C + 8, 8, M, C, v[0], v[1], rb_, C + 16, 16, False, y2b, C + 32, 24, None, rs, rh)
    check_apply(x, v[0], v[1], res, rs, rh, False, y2, None, "bn_apply deferred residual")
    assert _outside_untouched(y2b, 24, C)

    ym.copy_(y)   # the mask operand: the stored y, in yet another buffer
    xhat = (xd - v[2].double()) * v[3].double()
    dyr = R.masked(dy, ym)
    part = torch.empty(nblk, 2, C, device=DEV)
    nb.C.bn_bwd_reduce(dyb, C + 40, 8, ymb, 2 * C + 8, C, xb, C + 8, 8, M, C, v[2], v[3], part, nblk)
    check_sums(part, nblk, R.bwd_reduce(dy, ym, x, v[2], v[3]), (dyr.abs().sum(0), (dyr * xhat).abs().sum(0)), L,
               (1, 4), "bn_bwd_reduce")
    dg0, db0 = torch.randn(C, generator=g, device=DEV), torch.randn(C, generator=g, device=DEV)
    dg, db, coef = dg0.clone(), db0.clone(), torch.empty(3, C, device=DEV)
    nb.C.bn_bwd_finalize(part, nblk, C, float(M), gamma, v[2], v[3], dg, db, coef)
    check_bwd_finalize(part, nblk, 1, False, M, gamma, v[2], v[3], dg0, db0, dg, db, coef, "bn_bwd_finalize")
    # dx / dyr_out are dense [M][C]: two rows more, which must keep the sentinel
    dx = torch.full((M + 2, C), SENT, device=DEV, dtype=dtype)
    dyo = torch.full((M + 2, C), SENT, device=DEV, dtype=dtype)
    nb.C.bn_bwd_apply(dyb, C + 40, 8, ymb, 2 * C + 8, C, xb, C + 8, 8, M, C, coef, dx, dyo)
    check_bwd_apply(dy, ym, x, coef, dx[:M], dyo[:M], "bn_bwd_apply")
    assert bool((dx[M:] == SENT).all()) and bool((dyo[M:] == SENT).all())
    assert _outside_untouched(ymb, C, C) and bool((ym == y).all())


# ------------------------------------------------------------------ C. apply modes
def _special_row(x, res, scale, shift, rscale, rshift, row):
    """Channels 0..5 of `row`: pre-activations exactly -0.0, +0, +2^-100, -2^-100, a negative sum,
    and -0.0 + +0 (2^-100 is normal in bf16 and fp32: no denormal handling involved)."""
    tiny = 2.0 ** -100
    scale[:8], rscale[:8] = 1.0, 1.0
    shift[:8], rshift[:8] = 0.0, 0.0
    shift[0] = shift[5] = rshift[0] = -0.0
    xs = torch.tensor([-0.0, 0.0, tiny, -tiny, -1.0, -0.0], device=DEV)
    rs = torch.tensor([-0.0, 0.0, 0.0, 0.0, 0.5, 0.0], device=DEV)
    x[row, :6] = xs.to(x.dtype)
    res[row, :6] = rs.to(res.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 37, 1031])
@pytest.mark.parametrize("C", [8, 24, 72, 2048])
def test_apply_modes(nb, C, M, dtype):
    g = _gen(C * 7 + M)
    _, x = _sliced(M, C, C, 0, dtype, g)
    _, res = _sliced(M, C, C, 0, dtype, g)
    scale, shift = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    rscale, rshift = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    row = M // 2
    _special_row(x, res, scale, shift, rscale, rshift, row)
    for kind in ("none", "act", "deferred"):
        r, rs, rh = (None, None, None) if kind == "none" else (res, None, None) if kind == "act" else \
            (res, rscale, rshift)
        for relu in (False, True):
            for with_bits in (False, True):
                y = torch.full((M, C), SENT, device=DEV, dtype=dtype)
                bits = torch.full((M, C // 8), 0xA5, dtype=torch.uint8, device=DEV) if with_bits else None
                nb.C.bn_apply(x, C, 0, M, C, scale, shift, r, C if r is not None else 0, 0, relu, y, C, 0, bits,
                              rs, rh)
                what = f"res={kind} relu={relu} bits={with_bits}"
                check_apply(x, scale, shift, r, rs, rh, relu, y, bits, what)
                sp = y[row].float()
                # the zeros are zeros (the reference has mag == 0 there: no slack at all)
                assert sp[0].item() == 0.0 and sp[1].item() == 0.0 and sp[5].item() == 0.0, what
                if not relu:   # -0.0 reaches the store, and its mask bit is clear
                    assert bool(torch.signbit(sp[0])) and not bool(torch.signbit(sp[1])), what
                    assert sp[2].item() == 2.0 ** -100 and sp[3].item() == -(2.0 ** -100), what
                    assert sp[4].item() == (-1.0 if kind == "none" else -0.5), what
                else:
                    assert sp[2].item() == 2.0 ** -100 and sp[3].item() == 0.0 and sp[4].item() == 0.0, what
                if with_bits:
                    assert int(bits[row, 0].item()) & 0x3F == 0b000100, what


# ------------------------------------------------------------------ D. grid-stride second trip
def test_grid_stride_second_trip(nb):
    """More work items than the 8192 x 256 threads of the capped grid: the loops of bn_apply and
    bn_bwd_apply take a second trip for the last 37 rows."""
    C, M, dtype = 64, 8192 * 256 // 8 + 37, BF16
    g = _gen(5)
    _, x = _sliced(M, C, C, 0, dtype, g)
    _, res = _sliced(M, C, C, 0, dtype, g)
    _, dy = _sliced(M, C, C, 0, dtype, g)
    scale, shift = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    coef = torch.randn(3, C, generator=g, device=DEV)
    y = torch.full((M, C), SENT, device=DEV, dtype=dtype)
    bits = torch.full((M, C // 8), 0xA5, dtype=torch.uint8, device=DEV)
    nb.C.bn_apply(x, C, 0, M, C, scale, shift, res, C, 0, True, y, C, 0, bits, None, None)
    check_apply(x, scale, shift, res, None, None, True, y, bits, "bn_apply")
    dx = torch.full((M, C), SENT, device=DEV, dtype=dtype)
    dyo = torch.full((M, C), SENT, device=DEV, dtype=dtype)
    nb.C.bn_bwd_apply(dy, C, 0, y, C, 0, x, C, 0, M, C, coef, dx, dyo)
    check_bwd_apply(dy, y, x, coef, dx, dyo, "bn_bwd_apply")


# ------------------------------------------------------------------ E. forward finalize
FIN_CASES = [(T, C) for C in (8, 72) for T in (1, 63, 64, 65, 511, 512, 513, 2049, 2100)] + [(512, 2048), (513, 2048)]


def _fwd_partials(T, C, g, per=128.0):
    """Per-tile {sum x, sum x^2} of `per` values each; channel 3 has zero variance (1.5 throughout,
    exact sums), channel 5 a mean of 100 standard deviations."""
    m = torch.randn(T, 1, C, generator=g, device=DEV) * 3 + _mu(C, g)
    m[:, :, 5] = 100 + torch.randn(T, 1, generator=g, device=DEV) / math.sqrt(per)
    q = m * m + torch.rand(T, 1, C, generator=g, device=DEV)
    q[:, :, 5] = m[:, :, 5] ** 2 + 1
    m[:, :, 3], q[:, :, 3] = 1.5, 2.25
    return torch.cat([m, q], 1) * per


def _run_fwd(nb, st, T, C, count, gamma, beta, rm0, rv0, mom):
    v = torch.full((4, C), float("nan"), device=DEV)
    rm, rv = (rm0.clone(), rv0.clone()) if rm0 is not None else (None, None)
    nb.C.bn_finalize(st, T, C, float(count), gamma, beta, rm, rv, mom, EPS, v[0], v[1], v[2], v[3])
    return v, rm, rv


@pytest.mark.parametrize("T,C", FIN_CASES)
def test_forward_finalize(nb, T, C):
    """Synthetic partials through the direct kernel (T <= 512) and the ticket kernel (beyond), at channel
    counts that are no multiple of the 16- and 64-channel groups."""
    g = _gen(T * 3 + C)
    st = _fwd_partials(T, C, g)
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    rm0, rv0 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    v, rm, rv = _run_fwd(nb, st, T, C, T * 128, gamma, beta, rm0, rv0, 0.1)
    f = check_fwd_finalize(st, T, T * 128, gamma, beta, rm0, rv0, 0.1, v, rm, rv, f"T={T} C={C}")
    assert f["var"][3].item() == 0.0   # the zero-variance channel is one: invstd = eps^-1/2 there


@pytest.mark.parametrize("T", [65, 513])
@pytest.mark.parametrize("C", [8, 72])
def test_forward_finalize_variants(nb, T, C):
    g = _gen(T + C)
    st = _fwd_partials(T, C, g)
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    rm0, rv0 = torch.randn(C, generator=g, device=DEV) * 2, torch.rand(C, generator=g, device=DEV) * 3 + 0.1
    n = T * 128
    for mom in (0.1, 1.0):   # running statistics from random values
        v, rm, rv = _run_fwd(nb, st, T, C, n, gamma, beta, rm0, rv0, mom)
        check_fwd_finalize(st, T, n, gamma, beta, rm0, rv0, mom, v, rm, rv, f"momentum={mom}")
    for ga, be in ((None, None), (gamma, None), (None, beta)):
        v, rm, rv = _run_fwd(nb, st, T, C, n, ga, be, rm0, rv0, 0.1)
        check_fwd_finalize(st, T, n, ga, be, rm0, rv0, 0.1, v, rm, rv, f"gamma={ga is not None} beta={be is not None}")
    v, _, _ = _run_fwd(nb, st, T, C, n, gamma, beta, None, None, 0.1)   # no running statistics
    check_fwd_finalize(st, T, n, gamma, beta, None, None, 0.1, v, None, None, "no running stats")
    # count == 1: the partials of one value per channel, spread over T rows -> unbiased = biased
    st1 = st / n
    v, rm, rv = _run_fwd(nb, st1, T, C, 1, gamma, beta, rm0, rv0, 0.1)
    f = check_fwd_finalize(st1, T, 1, gamma, beta, rm0, rv0, 0.1, v, rm, rv, "count=1")
    assert torch.equal(f["unbiased"], f["var"])


def test_ticket_calls_back_to_back(nb):
    """Ticket-path launches queued on one stream with different T, C and data: every one starts from
    tickets the launch before it has reset."""
    g = _gen(11)
    runs = []
    for T, C in ((513, 72), (2100, 72), (600, 2048), (1029, 8), (513, 72)):
        st = _fwd_partials(T, C, g)
        gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
        rm0, rv0 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        runs.append((st, T, C, gamma, beta, rm0, rv0) + _run_fwd(nb, st, T, C, T * 128, gamma, beta, rm0, rv0, 0.1))
    for st, T, C, gamma, beta, rm0, rv0, v, rm, rv in runs:
        check_fwd_finalize(st, T, T * 128, gamma, beta, rm0, rv0, 0.1, v, rm, rv, f"T={T} C={C}")


# ------------------------------------------------------------------ F. backward finalize
def _bwd_case(T, C, ns, g):
    part = torch.randn(T, ns, C, generator=g, device=DEV) * 4 + _mu(C, g)
    mean = _mu(C, g)
    invstd = torch.rand(C, generator=g, device=DEV) * 2 + 0.3
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    dg0, db0 = torch.randn(C, generator=g, device=DEV) * 5, torch.randn(C, generator=g, device=DEV) * 5
    return part, mean, invstd, gamma, dg0, db0


@pytest.mark.parametrize("T,C", FIN_CASES)
def test_backward_finalize(nb, T, C):
    """mode 1 of every column-reduce path: bn_bwd_finalize (xhat sums) and bn_bwd_finalize_fused
    (raw_z; ns 2 and 3, k2 1 and 2 with the unused row full of NaN), into non-zero dgamma / dbeta."""
    g = _gen(T * 5 + C)
    count = float(T * 16)
    part, mean, invstd, gamma, dg0, db0 = _bwd_case(T, C, 2, g)
    dg, db, coef = dg0.clone(), db0.clone(), torch.full((3, C), float("nan"), device=DEV)
    nb.C.bn_bwd_finalize(part, T, C, count, gamma, mean, invstd, dg, db, coef)
    check_bwd_finalize(part, T, 1, False, count, gamma, mean, invstd, dg0, db0, dg, db, coef, "ns=2 xhat")
    for ns, k2 in ((2, 1), (3, 1), (3, 2)):
        part, mean, invstd, gamma, dg0, db0 = _bwd_case(T, C, ns, g)
        if ns == 3:
            part[:, 3 - k2] = float("nan")   # the row of the other BN consumer: nothing may read it
        dg, db, coef = dg0.clone(), db0.clone(), torch.full((3, C), float("nan"), device=DEV)
        nb.C.bn_bwd_finalize_fused(part, k2, C, count, gamma, mean, invstd, dg, db, coef)
        check_bwd_finalize(part, T, k2, True, count, gamma, mean, invstd, dg0, db0, dg, db, coef,
                           f"fused ns={ns} k2={k2}")


@pytest.mark.parametrize("T", [65, 513])
@pytest.mark.parametrize("C", [8, 72])
def test_backward_finalize_variants(nb, T, C):
    g = _gen(T * 9 + C)
    count = float(T * 16)
    part, mean, invstd, gamma, dg0, db0 = _bwd_case(T, C, 2, g)
    # gamma None
    dg, db, coef = dg0.clone(), db0.clone(), torch.empty(3, C, device=DEV)
    nb.C.bn_bwd_finalize(part, T, C, count, None, mean, invstd, dg, db, coef)
    check_bwd_finalize(part, T, 1, False, count, None, mean, invstd, dg0, db0, dg, db, coef, "gamma None")
    dg, db, coef = dg0.clone(), db0.clone(), torch.empty(3, C, device=DEV)
    nb.C.bn_bwd_finalize_fused(part, 1, C, count, None, mean, invstd, dg, db, coef)
    check_bwd_finalize(part, T, 1, True, count, None, mean, invstd, dg0, db0, dg, db, coef, "fused gamma None")
    # coef None: the accumulators alone (and without mean / invstd in the xhat form)
    dg, db = dg0.clone(), db0.clone()
    nb.C.bn_bwd_finalize(part, T, C, count, gamma, None, None, dg, db, None)
    check_bwd_finalize(part, T, 1, False, count, gamma, mean, invstd, dg0, db0, dg, db, None, "coef None")
    dg, db = dg0.clone(), db0.clone()
    nb.C.bn_bwd_finalize_fused(part, 1, C, count, gamma, mean, invstd, dg, db, None)
    check_bwd_finalize(part, T, 1, True, count, gamma, mean, invstd, dg0, db0, dg, db, None, "fused coef None")
    # no accumulators: the coefficients alone; count == 1
    coef = torch.empty(3, C, device=DEV)
    nb.C.bn_bwd_finalize(part, T, C, 1.0, gamma, mean, invstd, None, None, coef)
    check_bwd_finalize(part, T, 1, False, 1.0, gamma, mean, invstd, None, None, None, None, coef, "count=1")
    assert bool(torch.isfinite(coef).all())


# ------------------------------------------------------------------ G. dual_dgrad_weights
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [8, 72, 256, 264])
def test_dual_dgrad_weights(nb, K, dtype):
    Cr = 5
    g = _gen(K)
    W = torch.randn(Cr, K, generator=g, device=DEV).to(dtype)
    coef = torch.randn(3, K, generator=g, device=DEV)
    w2 = torch.full((Cr + 1, 2 * K), SENT, device=DEV, dtype=dtype)
    b = torch.full((Cr + 1,), SENT, device=DEV)
    nb.C.dual_dgrad_weights(W, Cr, K, coef, w2, b)
    ref, bref, babs = R.dual_weights(W, coef[0], coef[1], coef[2])
    err, tol = (w2[:Cr].double() - ref).abs(), R.store_tol(ref, dtype) + 1 * U * ref.abs()   # one product
    assert _le(err, tol), f"w2: {_worst(err, tol)}"
    err, tol = (b[:Cr].double() - bref).abs(), (K / 256 + 10) * U * babs
    assert _le(err, tol), f"b: {_worst(err, tol)}"
    assert bool((w2[Cr] == SENT).all()) and b[Cr].item() == SENT


# ------------------------------------------------------------------ H. the Python entry points
@pytest.mark.parametrize("dtype", DTYPES)
def test_entry_points_bit_identical_to_staged_calls(dtype):
    """NativeBackend.bn_stats / bn_finalize / bn_apply / bn_bwd / channel_sum on sliced Acts give the
    bits of the staged nb.C calls the cases above check (same kernels, same order, deterministic)."""
    nb = NativeBackend(DEV, dtype)
    Cc = nb.C
    C, N, H, W = 24, 3, 21, 23
    M = N * H * W
    g = _gen(24)
    xb, _ = _sliced(M, C, C + 8, 8, dtype, g, _mu(C, g))
    rb_, _ = _sliced(M, C, C + 16, 16, dtype, g)
    dyb, _ = _sliced(M, C, C + 40, 8, dtype, g, _mu(C, g))
    x, res, dy = Act(xb, N, H, W, C, 8), Act(rb_, N, H, W, C, 16), Act(dyb, N, H, W, C, 8)
    gamma, beta = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)
    rs, rh = torch.rand(C, generator=g, device=DEV) + 0.5, torch.randn(C, generator=g, device=DEV)

    part, nblk = nb.bn_stats(x)
    assert nblk == Cc.reduce_blocks(M, C) and tuple(part.shape) == (nblk, 2, C)
    part2 = torch.empty_like(part)
    Cc.bn_stats(xb, M, C, C + 8, 8, part2, nblk)
    assert torch.equal(part, part2)

    outs = []
    for via_backend in (True, False):
        v = torch.empty(4, C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        if via_backend:
            nb.bn_finalize(part, nblk, C, M, gamma, beta, rm, rv, 0.1, EPS, v[0], v[1], v[2], v[3])
        else:
            Cc.bn_finalize(part, nblk, C, float(M), gamma, beta, rm, rv, 0.1, EPS, v[0], v[1], v[2], v[3])
        outs.append((v, rm, rv))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    v = outs[0][0]

    for r in (None, res, Deferred.bn(res, rs, rh)):
        ya = Act(torch.full((M, 2 * C), SENT, device=DEV, dtype=dtype), N, H, W, C, C - 8)
        yb = torch.full((M, 2 * C), SENT, device=DEV, dtype=dtype)
        bits_a = torch.empty(M, C // 8, dtype=torch.uint8, device=DEV)
        bits_b = torch.empty_like(bits_a)
        nb.bn_apply(x, v[0], v[1], r, True, ya, mbits=bits_a)
        Cc.bn_apply(xb, C + 8, 8, M, C, v[0], v[1], rb_ if r is not None else None, C + 16 if r is not None else 0,
                    16 if r is not None else 0, True, yb, 2 * C, C - 8, bits_b,
                    rs if isinstance(r, Deferred) else None, rh if isinstance(r, Deferred) else None)
        assert torch.equal(ya.buf, yb) and torch.equal(bits_a, bits_b)
    y = ya   # relu(bn(x) + bn(res)): the mask of the backward, sliced

    dg_a, db_a = torch.ones(C, device=DEV), torch.ones(C, device=DEV)
    dx_a, dyo_a = Act.empty(N, H, W, C, dtype, DEV), Act.empty(N, H, W, C, dtype, DEV)
    nb.bn_bwd(dy, y, x, v[2], v[3], gamma, dg_a, db_a, dx_a, dyo_a)
    dg_b, db_b, coef = torch.ones(C, device=DEV), torch.ones(C, device=DEV), torch.empty(3, C, device=DEV)
    bp = torch.empty(nblk, 2, C, device=DEV)
    Cc.bn_bwd_reduce(dyb, C + 40, 8, y.buf, 2 * C, C - 8, xb, C + 8, 8, M, C, v[2], v[3], bp, nblk)
    Cc.bn_bwd_finalize(bp, nblk, C, float(M), gamma, v[2], v[3], dg_b, db_b, coef)
    dx_b, dyo_b = torch.empty(M, C, device=DEV, dtype=dtype), torch.empty(M, C, device=DEV, dtype=dtype)
    Cc.bn_bwd_apply(dyb, C + 40, 8, y.buf, 2 * C, C - 8, xb, C + 8, 8, M, C, coef, dx_b, dyo_b)
    assert torch.equal(dg_a, dg_b) and torch.equal(db_a, db_b)
    assert torch.equal(dx_a.buf, dx_b) and torch.equal(dyo_a.buf, dyo_b)
    # and the staged calls are themselves right
    check_bwd_apply(dyb[:, 8:8 + C], R.view(y), R.view(x), coef, dx_b, dyo_b, "bn_bwd_apply")

    acc_a = torch.full((C,), 2.5, device=DEV)
    acc_b = acc_a.clone()
    nb.channel_sum(x, acc_a)
    Cc.bn_bwd_reduce(xb, C + 8, 8, None, 0, 0, None, 0, 0, M, C, None, None, bp, nblk)
    Cc.bn_bwd_finalize(bp, nblk, C, float(M), None, None, None, None, acc_b, None)
    assert torch.equal(acc_a, acc_b)


# ------------------------------------------------------------------ argument checks
def test_entry_points_raise_on_unsupported_channel_counts(nb):
    """C < 8 and C > 2048 have no row map: a Python exception, not a division by zero in the host code."""
    for C in (4096, 4):
        a = Act(torch.zeros(6, max(C, 8), device=DEV, dtype=BF16), 1, 2, 3, C)
        with pytest.raises(RuntimeError):
            nb.C.reduce_blocks(6, C)
        with pytest.raises(RuntimeError):
            nb.bn_stats(a)
        with pytest.raises(RuntimeError):
            nb.channel_sum(a, torch.zeros(C, device=DEV))
        with pytest.raises(RuntimeError):
            nb.bn_bwd(a, None, a, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), None, None, None,
                      Act.empty(1, 2, 3, C, BF16, DEV))
    for M, C in ((0, 24), (-1, 24), (6, 12), (6, 0), (6, -8)):
        with pytest.raises(RuntimeError):
            nb.C.reduce_blocks(M, C)


def _good_calls(C, M, T):
    """One valid call of every BN binder, as ordered {argument: value} (the binders take positionals)."""
    t = lambda *s: torch.zeros(*s, device=DEV, dtype=BF16)   # noqa: E731
    f = lambda *s: torch.ones(*s, device=DEV)                 # noqa: E731
    sl = lambda p: {p: t(M, C), "ld" + p: C, p + "off": 0}    # noqa: E731
    no = lambda p: {p: None, "ld" + p: 0, p + "off": 0}       # noqa: E731
    fin = dict(gamma=f(C), mean=f(C), invstd=f(C), dgamma=f(C), dbeta=f(C), coef=f(3, C))
    prod = lambda: dict(z=t(M, C), mscale=f(C), mshift=f(C))   # noqa: E731  (the fused gradient producers)
    assert M == 10   # maxpool_bwd_bn below: a 1 x 2 x 5 input, 2x2 / s2 windows -> 1 x 1 x 2
    return {
        "outer_dgrad_bn": dict(dy=t(M, 8), lddy=8, M=M, C=C, w=t(C * 8), ldw=8, **prod(), dx=t(M, C)),
        "head_dgrad_bn": dict(dl=t(M, 8), lddl=8, K=3, M=M, C=C, w=t(C * 8), ldw=8, **prod(), dx=t(M, C)),
        "maxpool_bwd_bn": dict(dy=t(2, C), idx=torch.zeros(2 * C, dtype=torch.uint8, device=DEV), N=1, H=2, W=5, C=C,
                               k=2, stride=2, pad=0, OH=1, OW=2, **prod(), add=t(M, 2 * C), ldadd=2 * C, addoff=C,
                               dx=t(M, C)),
        "bn_stats": dict(x=t(M, C), M=M, C=C, ldx=C, xoff=0, partial=f(1, 2, C), nblk=1),
        "channel_sum": dict(x=t(M, C), M=M, C=C, ldx=C, xoff=0, out=f(C)),
        "bn_finalize": dict(partial=f(T, 2, C), T=T, C=C, count=30.0, gamma=f(C), beta=f(C), running_mean=f(C),
                            running_var=f(C), momentum=0.1, eps=EPS, scale=f(C), shift=f(C), save_mean=f(C),
                            save_invstd=f(C)),
        "bn_apply": dict(**sl("x"), M=M, C=C, scale=f(C), shift=f(C), **sl("res"), relu=True, **sl("y"),
                         mbits=torch.zeros(M, C // 8, dtype=torch.uint8, device=DEV), rscale=f(C), rshift=f(C)),
        "bn_bwd_reduce": dict(**sl("dy"), **sl("ymask"), **sl("x"), M=M, C=C, mean=f(C), invstd=f(C),
                              partial=f(1, 2, C), nblk=1),
        "bn_bwd_finalize": dict(partial=f(T, 2, C), T=T, C=C, count=30.0, **fin),
        "bn_bwd_finalize_fused": dict(partial=f(T, 3, C), k2=2, C=C, count=30.0, **fin),
        "bn_bwd_apply": dict(**sl("dy"), **sl("ymask"), **sl("x"), M=M, C=C, coef=f(3, C), dx=t(M, C),
                             dyr_out=t(M, C)),
    }, t, f, no


def test_binders_reject_out_of_range_operands(nb):
    """Every argument the kernels would follow outside a tensor is refused before any launch: each call
    below is a valid call with exactly one argument (or one operand's slice) made bad, so none reaches a
    kernel.  The valid calls themselves go through."""
    C, M, T = 24, 10, 3
    good, t, f, no = _good_calls(C, M, T)
    short, wide = f(C - 1), t(M, C + 8)
    bad = []
    for name in ("bn_stats", "channel_sum", "bn_bwd_reduce"):               # the row-map kernels
        bad += [(name, dict(C=c)) for c in (4, 12, 0, 2056, 4096)] + [(name, dict(M=0))]
    for name in ("bn_apply", "bn_bwd_apply"):                               # one thread per 8 channels
        bad += [(name, dict(C=c)) for c in (4, 12, 0)] + [(name, dict(M=0))]
    # partials smaller than the launch writes or reads
    bad += [("bn_stats", dict(nblk=2)), ("bn_stats", dict(nblk=0)), ("bn_bwd_reduce", dict(nblk=2)),
            ("bn_bwd_reduce", dict(nblk=0)), ("bn_stats", dict(partial=f(1, 2, C).double()))]
    for name in ("bn_finalize", "bn_bwd_finalize"):
        bad += [(name, dict(T=T + 1)), (name, dict(T=0)), (name, dict(count=0.0)), (name, dict(C=C + 8))]
    bad += [("bn_bwd_finalize_fused", d) for d in (
        dict(partial=f(T, 3 * C)), dict(partial=f(T, 4, C)), dict(partial=f(T, 1, C), k2=1), dict(k2=3), dict(k2=0),
        dict(partial=f(T, 2, C)), dict(C=C - 8), dict(count=0.0))]
    # x without mean / invstd; the coefficients without them
    bad += [("bn_bwd_reduce", dict(mean=None)), ("bn_bwd_reduce", dict(invstd=None)),
            ("bn_bwd_finalize", dict(mean=None)), ("bn_bwd_finalize", dict(invstd=None))]
    # per-channel vectors shorter than C (3C for coef), or not fp32
    vectors = {"bn_finalize": ("gamma", "beta", "running_mean", "running_var", "scale", "shift", "save_mean",
                               "save_invstd"),
               "bn_apply": ("scale", "shift", "rscale", "rshift"),
               "bn_bwd_reduce": ("mean", "invstd"),
               "bn_bwd_finalize": ("gamma", "mean", "invstd", "dgamma", "dbeta"),
               "bn_bwd_finalize_fused": ("gamma", "mean", "invstd", "dgamma", "dbeta"),
               "channel_sum": ("out",)}
    for name, vs in vectors.items():
        bad += [(name, {v: short}) for v in vs] + [(name, {vs[0]: f(C).double()})]
    bad += [(name, dict(coef=f(3 * C - 1))) for name in ("bn_bwd_finalize", "bn_bwd_finalize_fused", "bn_bwd_apply")]
    bad += [("bn_finalize", dict(running_var=None)), ("bn_finalize", dict(running_mean=None)),
            ("bn_apply", dict(rshift=None)), ("bn_apply", dict(**no("res"))),   # rscale without a residual
            ("bn_apply", dict(mbits=torch.zeros(M - 1, C // 8, dtype=torch.uint8, device=DEV)))]
    # sliced operands: off + C > ld, a negative offset, a buffer shorter than (M - 1) * ld + off + C, another dtype
    slices = {"bn_stats": ("x",), "channel_sum": ("x",), "bn_apply": ("x", "res", "y"),
              "bn_bwd_reduce": ("dy", "ymask", "x"), "bn_bwd_apply": ("dy", "ymask", "x")}
    for name, ps in slices.items():
        for p in ps:
            bad += [(name, {p: wide, "ld" + p: C + 8, p + "off": 16}),       # off + C > ld
                    (name, {p: wide, "ld" + p: C + 8, p + "off": -8}),
                    (name, {p: t(M - 1, C)}),                                # a row short
                    (name, {"ld" + p: C + 8}),                               # rows further apart than the buffer has
                    (name, {p: t(M, C), "ld" + p: C + 8, p + "off": 8})]     # off + C <= ld, but past the end
            if name not in ("bn_stats", "channel_sum") or p != "x":
                bad.append((name, {p: t(M, C).float()}))                     # storage types differ
    bad += [("bn_bwd_apply", dict(dx=t(M - 1, C))), ("bn_bwd_apply", dict(dyr_out=t(M - 1, C))),
            ("bn_bwd_apply", dict(dx=t(M, C).float()))]
    # the fused gradient producers: z / dx a row short, mscale a channel short; the pool's add slice past its row
    for name in ("outer_dgrad_bn", "head_dgrad_bn", "maxpool_bwd_bn"):
        bad += [(name, dict(z=t(M - 1, C))), (name, dict(dx=t(M - 1, C))), (name, dict(mscale=short))]
    bad += [("maxpool_bwd_bn", dict(addoff=C + 8))]

    def call(name, over):
        a = dict(good[name])
        assert set(over) <= set(a), (name, over)
        a.update(over)
        return getattr(nb.C, name)(*a.values())

    for name, over in bad:
        with pytest.raises(RuntimeError):
            call(name, over)
            pytest.fail(f"{name} accepted {({k: getattr(v, 'shape', v) for k, v in over.items()})}")
    for name in good:   # ... and the calls these were cut from are valid
        call(name, {})
    torch.cuda.synchronize()
    y = good["bn_apply"]["y"]   # relu(0 * 1 + 1 + (0 * 1 + 1))
    assert bool((y == 2).all()) and bool((good["bn_apply"]["mbits"] == 0xFF).all())
