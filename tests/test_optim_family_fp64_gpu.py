"""The kernels that touch the master weights (csrc/kernels/optim.hip, cast.hip, util.hip), reached through
NativeBackend, against the fp64 reference of tests/optim_ref.py at their edge shapes: every flat size at
which a loop changes (vector body, < 4 tail, more than one block, the second trip of each capped grid),
the full product of the SGD settings, Adam / AdamW with every clip, write-back and step-count mode,
misaligned operands (the element loop, bit-equal to the vector loop), the gradient norm's three loops and
its coefficient sizes, fill / add / gather, and every branch of the weight re-layout from both sides.

Every operand is carved out of a larger buffer of sentinels that must survive the call.  One update per
case from identical fp32 state, compared elementwise with fp64 evaluated on the same fp32 inputs.  What
only selects, copies, scales once or rounds to bf16 is exact (bit for bit; NaN equals NaN).  The bounds of
the rest count roundings (profiles/optim_tests/README.md derives each): u = 2^-24, g(k) = k u / (1 - k u),
eta = 2^-149 (a result below the normal range), M the fp64 sum of the absolute terms of an element:

* SGD     m: g(2[wd] + 3[not first]) Mm;  p: g(that + 2[nesterov] + 2) Mp
* Adam    m: g(kg + 4) Mm + 4 eta;  v: g(2 kg + 4) Mv + 5 eta, kg = [clip] + 2[L2 decay];
          p: 3 u |p1| [AdamW] + u (|p1| + |upd|) + |upd| (g(4) + dD / D) + (lr / bc1) dm / D, dD from dv through
          the square root, its division by sqrt(bc2) and the sum with eps (5 more roundings)
* norm    (g(k) / 2 + u) norm, k = accumulations per lane + 2 + 6 + 3 (lane sums, wave tree, block sum);
          coefficient: coef (dnorm / (norm + 1e-6) + 3 u)

Set DLMPI_OPTIM_RATIOS to a file name to have the largest err / bound of every bounded comparison written there.
"""
import itertools
import math
import os
import zlib

import pytest
import torch

import optim_ref as R
from deeplearning_mpi_amd.ops.backend import NativeBackend

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
ETA = 2.0 ** -149
SLACK = 1 + 2.0 ** -10   # second-order terms of the first-order propagation (Adam's p, the norm)
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 640.0      # exact in bf16; no result below comes near it
ISENT = 77777
PAD = 64          # sentinel elements on either side of an operand (a multiple of 4: 16-byte alignment stays)

NS = [1, 3, 4, 5, 7, 255, 256, 257, 1023, 1025]
# blocks_for / ew_blocks cap a grid at 4096 blocks of 256 threads:
N2V = 4 * 4096 * 256 + 4 * 256 + 3   # float4 loops (sgd, adam, fill): one more float4 for every lane of block 0, a tail of 3
N2S = 4096 * 256 + 257               # scalar loops (scale_, add_i64_, gather_)
# sumsq: 1024 x 256 lanes; lane 0 enters the four-loads-in-flight loop when n/4 > 3 * 262144
NSUM = 4 * (3 * 1024 * 256 + 1) + 3

RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_file():
    yield
    out = os.environ.get("DLMPI_OPTIM_RATIOS")
    if out:
        with open(out, "w") as f:
            for k in sorted(RATIOS):
                f.write(f"{RATIOS[k]:10.4f}  {k}\n")


@pytest.fixture(scope="module")
def nb():
    return NativeBackend(DEV)


@pytest.fixture(scope="module")
def nb32():
    return NativeBackend(DEV, torch.float32)


def _gen(*seed):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(seed).encode()))


def _gam(k):
    return k * U / (1 - k * U)


def _carve(vals, shift=0, sent=SENT):
    """(buffer of sentinels, the view of it that holds vals), the view `shift` elements off 16-byte alignment."""
    n = vals.numel()
    buf = torch.full((PAD + shift + n + PAD,), sent, dtype=vals.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[PAD + shift:PAD + shift + n]
    v.copy_(vals.reshape(-1))
    return buf, v


def _intact(buf, v, sent=SENT):
    off = (v.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:off] == sent).all()) and bool((buf[off + v.numel():] == sent).all())


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _prod32(x, c):
    """The fp32 product x * c, rounded once: the product of two floats is exact in fp64."""
    return (x.double() * float(c)).float()


def _le(err, tol, what):
    """err <= tol everywhere (a NaN on either side fails); records the largest err / tol under `what`."""
    r = torch.nan_to_num(err / tol.clamp_min(1e-300), nan=float("inf"))
    r = torch.where((err == 0) & (tol == 0), torch.zeros_like(r), r)
    worst = float(r.max()) if r.numel() else 0.0
    RATIOS[what] = max(RATIOS.get(what, 0.0), worst)
    ok = bool((err <= tol).all())
    assert ok, f"{what}: worst err / bound = {worst:.4g} at {int(r.argmax())} of {r.numel()}"


# ------------------------------------------------------------------ shared state (computed once, never changed)
_STATE = {}
G_SPECIAL = [0.0, 1e-30, -1e-30, 1e-20, -1e-20, 1e15, -1e15]


def _state(n):
    """fp32 (p, g, m, v, g_adam) of n elements.  |p| spans 1 .. 1e-4 and has exact zeros, so an error of the step
    is not hidden under the rounding of a large p; v >= 0; g_adam carries 0, +-1e-30 and +-1e-20 (g^2 underflows) and
    +-1e15 (fp32 g^2 still finite)."""
    if n not in _STATE:
        g = _gen("state", n)
        i = torch.arange(n, device=DEV)
        p = torch.randn(n, generator=g, device=DEV) * (10.0 ** -(i % 5).float())
        p[i % 11 == 3] = 0.0
        gr = torch.randn(n, generator=g, device=DEV) * 0.1
        gr[i % 7 == 2] = 0.0
        m = torch.randn(n, generator=g, device=DEV) * 0.1
        v = torch.rand(n, generator=g, device=DEV) * 0.01
        ga = gr.clone()
        for j, s in enumerate(G_SPECIAL):
            ga[i % 29 == j + 1] = s
        _STATE[n] = (p, gr, m, v, ga)
    return _STATE[n]


def _scalar(x):
    buf, v = _carve(torch.tensor([x], dtype=F32, device=DEV))
    return buf, v


# ------------------------------------------------------------------ SGD
LR, WD = R.f32(0.05), R.f32(1e-4)


def _sgd_tols(d, wd, momentum, nesterov, first):
    kd = 2 if wd != 0 else 0                 # wd * p, the sum
    km = kd + (0 if first else 3)            # 1 - dampening, two products, one sum (FMA only removes one)
    if momentum != 0:
        kd = km + (2 if nesterov else 0)     # momentum * m, the sum
    return (_gam(km) * d["Mm"] if momentum != 0 else None), _gam(kd + 2) * d["Mp"]   # lr * d, the difference


def _run_sgd(nb, n, momentum, dampening, wd, nesterov, first, skip=None, alias=False, shifts=(0, 0, 0), g=None):
    """One call on carved copies of the shared state -> (p, m or None, buffers intact)."""
    p0, g0, m0 = _state(n)[:3]
    g0 = g0 if g is None else g
    pb, p = _carve(p0, shifts[0])
    gb, gv = _carve(g0, shifts[1])
    mb, m = (pb, p) if alias else _carve(m0, shifts[2])
    sb = sv = None
    if skip is not None:
        sb, sv = _scalar(skip)
    nb.sgd(p, gv, m, LR, momentum, dampening, wd, nesterov, first, sv)
    torch.cuda.synchronize()
    ok = _intact(pb, p) and _intact(gb, gv) and _intact(mb, m) and _biteq(gv, g0)
    if sb is not None:
        ok = ok and _intact(sb, sv) and (_biteq(sv, torch.tensor([skip], device=DEV)))
    return p, (None if alias else m), ok


SGD_CONFIGS = list(itertools.product((0.0, 0.9), (0.0, 0.1), (0.0, WD), (False, True), (True, False)))


@pytest.mark.parametrize("momentum,dampening,wd,nesterov,first", SGD_CONFIGS)
def test_sgd(nb, momentum, dampening, wd, nesterov, first):
    mom, damp = R.f32(momentum), R.f32(dampening)
    what = f"sgd mom={momentum} damp={dampening} wd={wd:.0e} nesterov={int(nesterov)} first={int(first)}"
    for n in NS + [N2V]:
        p0, g0, m0 = _state(n)[:3]
        rp, rm, d = R.sgd(p0, g0, m0, LR, mom, damp, wd, nesterov, first, detail=True)
        tm, tp = _sgd_tols(d, wd, mom, nesterov, first)
        for alias in ((False, True) if momentum == 0 else (False,)):   # optim.SGD passes m = p without momentum
            p, m, ok = _run_sgd(nb, n, mom, damp, wd, nesterov, first, alias=alias)
            assert ok, (n, alias)
            _le((p.double() - rp).abs(), tp, what + " p")
            if momentum == 0:
                assert alias or _biteq(m, m0), n   # m is not touched
            else:
                _le((m.double() - rm).abs(), tm, what + " m")


@pytest.mark.parametrize("skip", [None, 0.0, -0.0, 1.0, float("nan")])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_skip_flag(nb, skip, momentum):
    mom = R.f32(momentum)
    for n in (5, 1025, N2V):
        p0, g0, m0 = _state(n)[:3]
        p, m, ok = _run_sgd(nb, n, mom, 0.0, WD, True, False, skip=skip)
        assert ok
        if skip is not None and skip != 0.0:   # 1.0 and NaN
            assert _biteq(p, p0) and _biteq(m, m0), n
            continue
        rp, rm, d = R.sgd(p0, g0, m0, LR, mom, 0.0, WD, True, False, skip=skip, detail=True)
        tm, tp = _sgd_tols(d, WD, mom, True, False)
        _le((p.double() - rp).abs(), tp, "sgd skip-flag p")
        if momentum != 0:
            _le((m.double() - rm).abs(), tm, "sgd skip-flag m")
        else:
            assert _biteq(m, m0)


def _classes_match(x, ref):
    """NaN at the same places, infinities of the same sign at the same places -> the mask of the finite rest."""
    x = x.double()
    assert torch.equal(x.isnan(), ref.isnan())
    assert torch.equal(x.isinf(), ref.isinf())
    inf = ref.isinf()
    assert torch.equal(x[inf] > 0, ref[inf] > 0)
    return ~(ref.isnan() | inf)


@pytest.mark.parametrize("momentum,nesterov,first", [(0.0, False, True), (0.9, False, True), (0.9, False, False),
                                                     (0.9, True, False)])
def test_sgd_nonfinite_gradients(nb, momentum, nesterov, first):
    mom = R.f32(momentum)
    for n in (7, 1025):
        p0, g0, m0 = _state(n)[:3]
        g = g0.clone()
        g[0], g[n // 2], g[n - 1] = float("inf"), float("-inf"), float("nan")
        if n > 7:
            g[4], g[5], g[6] = float("nan"), float("inf"), float("-inf")   # in the vector body
        p, m, ok = _run_sgd(nb, n, mom, 0.0, WD, nesterov, first, g=g)
        assert ok
        rp, rm, d = R.sgd(p0, g, m0, LR, mom, 0.0, WD, nesterov, first, detail=True)
        tm, tp = _sgd_tols(d, WD, mom, nesterov, first)
        fin = _classes_match(p, rp)
        assert int((~fin).sum()) == (3 if n == 7 else 6)
        _le((p.double() - rp).abs()[fin], tp[fin], "sgd non-finite g, the finite p")
        if momentum != 0:
            fin = _classes_match(m, rm)
            _le((m.double() - rm).abs()[fin], tm[fin], "sgd non-finite g, the finite m")


# ------------------------------------------------------------------ Adam
ALR, B1, B2, EPS, AWD = R.f32(1e-3), 0.9, 0.999, R.f32(1e-8), R.f32(1e-2)
CLIPS = [None, (1.0, 0.0), (0.5, 0.0), (0.5, 1.0), (1.0, 1.0)]
# (host corrections for update t) and (device count of the updates so far)
TSTEPS = [("host", 1), ("host", 2), ("host", 1000)] + [("dev", c) for c in (0, 1, 9, 99, 999, 99999)]


def _adam_tols(d, clip, wd, adamw):
    kg = (1 if clip is not None else 0) + (2 if (wd != 0 and not adamw) else 0)   # g * coef; wd * p and the sum
    tm = _gam(kg + 4) * d["Mm"] + 4 * ETA        # 1 - b1, g - m, the product, the sum
    tv = _gam(2 * kg + 4) * d["Mv"] + 5 * ETA    # v * b2, 1 - b2, two products, the sum; g enters twice
    sq, D, upd, p1 = d["sq"], d["den"], d["upd"].abs(), d["p1"].abs()
    # |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b)); sqrtf rounds once
    dsq = torch.minimum(tv.sqrt(), tv / sq.clamp_min(1e-300)) + U * sq + ETA
    r2 = math.sqrt(d["bc2"])
    dq = dsq / r2 + (sq / r2) * _gam(3)          # fl(bc2) under its root (half), sqrtf, the division
    dD = dq + U * D                              # + eps
    dupd = (ALR / d["bc1"]) * tm / D + upd * (_gam(4) + dD / D)   # fl(bc1), lr / bc1, the product with m, / D
    dp1 = _gam(3) * p1 if (adamw and wd != 0) else 0.0            # lr * wd, 1 - that, the product
    tp = (dp1 + dupd + U * (p1 + upd)) * SLACK                    # the difference
    return tp, tm, tv


def _run_adam(nb, n, wd, adamw, clip, wb, tmode, shifts=(0, 0, 0, 0)):
    """One call on carved copies of the shared state -> dict of the operands after it, the inputs and the update
    number; the sentinels around every operand are asserted here."""
    kind, tv = tmode
    t = tv if kind == "host" else tv + 1
    p0, _, m0, v0, g0 = _state(n)
    if t == 1:
        m0, v0 = torch.zeros_like(m0), torch.zeros_like(v0)
    pb, p = _carve(p0, shifts[0])
    gb, g = _carve(g0, shifts[1])
    mb, m = _carve(m0, shifts[2])
    vb, v = _carve(v0, shifts[3])
    cb = c = tb = ts = None
    if clip is not None:
        cb, c = _carve(torch.tensor(clip, dtype=F32, device=DEV))
    if kind == "dev":
        tb, ts = _scalar(float(tv))
    nb.adam(p, g, m, v, ALR, B1, B2, EPS, wd, adamw, 1 - B1 ** t, 1 - B2 ** t, c, ts, wb)
    torch.cuda.synchronize()
    assert _intact(pb, p) and _intact(gb, g) and _intact(mb, m) and _intact(vb, v), (n, shifts)
    skip = clip is not None and clip[1] != 0
    if cb is not None:
        assert _intact(cb, c) and _biteq(c, torch.tensor(clip, dtype=F32, device=DEV))
    if tb is not None:   # advanced by exactly 1 when the update applied, unchanged when skipped
        assert _intact(tb, ts) and float(ts[0]) == (tv if skip else tv + 1), (float(ts[0]), tv, skip)
    return {"p": p, "g": g, "m": m, "v": v, "p0": p0, "g0": g0, "m0": m0, "v0": v0, "t": t, "skip": skip}


def _check_adam(o, wd, adamw, clip, wb, what):
    if o["skip"]:
        assert all(_biteq(o[k], o[k + "0"]) for k in "pgmv"), what
        return
    coef = 1.0 if clip is None else clip[0]
    rp, rg, rm, rv, d = R.adam(o["p0"], o["g0"], o["m0"], o["v0"], ALR, R.f32(B1), R.f32(B2), EPS, wd, adamw, o["t"],
                               coef=coef, writeback=wb, bc_betas=(B1, B2), detail=True)
    tp, tm, tv = _adam_tols(d, clip, wd, adamw)
    _le((o["m"].double() - rm).abs(), tm, what + " m")
    _le((o["v"].double() - rv).abs(), tv, what + " v")
    _le((o["p"].double() - rp).abs(), tp, what + " p")
    if wb and coef != 1.0:   # the fp32 product, bit for bit
        assert _biteq(o["g"], _prod32(o["g0"], coef)) and torch.equal(o["g"].double(), rg), what
    else:
        assert _biteq(o["g"], o["g0"]), what


@pytest.mark.parametrize("wb", [False, True], ids=["nowb", "wb"])
@pytest.mark.parametrize("clip", CLIPS, ids=lambda c: "noclip" if c is None else f"clip{c[0]}-{int(c[1])}")
@pytest.mark.parametrize("wd,adamw", [(0.0, False), (0.0, True), (AWD, False), (AWD, True)],
                         ids=["wd0-l2", "wd0-w", "l2", "adamw"])
def test_adam(nb, wd, adamw, clip, wb):
    base = f"adam wd={wd:.0e} adamw={int(adamw)} clip={clip} wb={int(wb)}"
    for tmode in TSTEPS:
        for n in NS + [N2V]:
            o = _run_adam(nb, n, wd, adamw, clip, wb, tmode)
            _check_adam(o, wd, adamw, clip, wb, f"{base} t={tmode[0]}:{tmode[1]}")


def test_adam_writeback_equals_scale(nb):
    """The gradients a write-back leaves are the ones the separate scale pass stores for the same coefficient."""
    for n in NS + [N2V]:
        o = _run_adam(nb, n, 0.0, False, (0.5, 0.0), True, ("dev", 9))
        gb, g = _carve(o["g0"])
        cb, c = _carve(torch.tensor([0.5, float("nan")], device=DEV))
        nb.scale_(g, c)
        torch.cuda.synchronize()
        assert _intact(gb, g) and _biteq(g, o["g"]), n
    for coef in (0.37, 1e-3):   # not a power of two: the product rounds
        n = 1025
        p0, _, m0, v0, g0 = _state(n)
        cb, c = _carve(torch.tensor([coef, 0.0], device=DEV))
        bufs = [_carve(x) for x in (p0, g0, m0, v0)]
        nb.adam(*[b[1] for b in bufs], ALR, B1, B2, EPS, 0.0, False, 0.5, 0.5, c, None, True)
        gs = _carve(g0)
        nb.scale_(gs[1], c)
        torch.cuda.synchronize()
        assert _biteq(bufs[1][1], gs[1]) and _biteq(gs[1], _prod32(g0, float(c[0])))
        assert all(_intact(*b) for b in bufs) and _intact(*gs)


# ------------------------------------------------------------------ alignment: the element loop equals the vector loop
@pytest.mark.parametrize("first", [True, False])
def test_sgd_misaligned_operands_bit_equal(nb, first):
    mom, damp = R.f32(0.9), R.f32(0.1)
    for n in (7, 1025, N2V):
        pa, ma, ok = _run_sgd(nb, n, mom, damp, WD, True, first)
        assert ok
        for op in range(3):
            for s in (1, 2, 3):
                shifts = tuple(s if k == op else 0 for k in range(3))
                p, m, ok = _run_sgd(nb, n, mom, damp, WD, True, first, shifts=shifts)
                assert ok and _biteq(p, pa) and _biteq(m, ma), (n, shifts)


@pytest.mark.parametrize("wd,adamw", [(AWD, False), (AWD, True)], ids=["l2", "adamw"])
def test_adam_misaligned_operands_bit_equal(nb, wd, adamw):
    clip = (0.5, 0.0)
    for n in (7, 1025, N2V):
        a = _run_adam(nb, n, wd, adamw, clip, True, ("dev", 9))
        for op in range(4):
            for s in (1, 2, 3):
                shifts = tuple(s if k == op else 0 for k in range(4))
                o = _run_adam(nb, n, wd, adamw, clip, True, ("dev", 9), shifts=shifts)
                assert all(_biteq(o[k], a[k]) for k in "pgmv"), (n, shifts)


# ------------------------------------------------------------------ gradient norm and clip coefficient
def _sumsq_k(n, aligned):
    """Roundings on the way to one partial: FMA accumulations per lane (the scalar loop: a product and a sum each),
    (s0 + s1) + (s2 + s3), six wave-shuffle levels, three sums of the four wave results."""
    stride = 1024 * 256
    n4 = n // 4 if aligned else 0
    return -(-n4 // stride) + 2 * -(-(n - 4 * n4) // stride) + 2 + 6 + 3


def _norm_tols(n, rn, rc, aligned):
    tn = (0.5 * _gam(_sumsq_k(n, aligned)) + U) * rn * SLACK   # the root halves the sum's error; (float)sqrt
    return tn, rc * (tn / (rn + 1e-6) + 3 * U) * SLACK         # fl(1e-6), the sum, the division


def _run_norm(nb, g0, max_norm, shift=0, ncoef=2):
    gb, g = _carve(g0, shift)
    nbuf, nrm = _carve(torch.zeros(1, device=DEV))
    cb, c = _carve(torch.full((ncoef,), SENT, device=DEV))
    nb.grad_norm(g, max_norm, nrm, c)
    torch.cuda.synchronize()
    assert _intact(gb, g) and _biteq(g, g0) and _intact(nbuf, nrm) and _intact(cb, c)
    return float(nrm[0]), c


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_grad_norm(nb, shift):
    # (a norm near 1e-3, where the 1e-6 of the coefficient is a thousandth of it, at the small sizes)
    for n, scale in [(n, 1.0) for n in NS + [NSUM]] + [(n, 1e-3) for n in NS]:
        g0 = torch.randn(n, generator=_gen("norm", n), device=DEV) * scale
        rn = R.grad_norm(g0, 1.0)[0]
        for max_norm in (2.0 * rn, R.f32(rn), 0.5 * rn):   # above, equal to and below the norm
            _, rc, rf = R.grad_norm(g0, R.f32(max_norm))
            norm, c = _run_norm(nb, g0, max_norm, shift)
            tn, tc = _norm_tols(n, rn, rc, shift == 0)
            what = f"grad_norm {'aligned' if shift == 0 else 'unaligned'}"
            _le(torch.tensor([abs(norm - rn)]), torch.tensor([tn]), what + " norm")
            _le(torch.tensor([abs(float(c[0]) - rc)]), torch.tensor([tc]), what + " coef")
            assert float(c[1]) == rf == 0.0
        assert float(c[0]) < 1.0   # the last one clips


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_grad_norm_all_ones_is_exact(nb, shift):
    """Every partial sum is an integer below 2^24: the norm is the correctly rounded sqrt(n)."""
    for n in NS + [NSUM, N2S]:
        norm, c = _run_norm(nb, torch.ones(n, device=DEV), 1e9, shift)
        assert norm == R.f32(math.sqrt(n)), (n, norm)
        assert c.tolist() == [1.0, 0.0]


@pytest.mark.parametrize("n", [5, 1025, NSUM])
def test_grad_norm_nonfinite(nb, n):
    g0 = torch.randn(n, generator=_gen("normnf", n), device=DEV)
    for bad, want in ((float("inf"), [0.0, 1.0]), (float("-inf"), [0.0, 1.0]), (float("nan"), [1.0, 1.0])):
        for pos in (0, n - 1):
            g = g0.clone()
            g[pos] = bad
            norm, c = _run_norm(nb, g, 1.0)
            assert c.tolist() == want and (math.isnan(norm) if math.isnan(bad) else norm == float("inf"))
            assert (R.grad_norm(g, 1.0)[1], R.grad_norm(g, 1.0)[2]) == tuple(want)


def test_grad_norm_coef_sizes(nb):
    g0 = torch.randn(257, generator=_gen("coefsz"), device=DEV)
    rn, rc, _ = R.grad_norm(g0, 1.0)
    tc = _norm_tols(257, rn, rc, True)[1]
    for ncoef in (2, 3, 4, 5):
        for g, flag in ((g0, 0.0), (torch.cat([g0[:5], g0.new_tensor([float("inf")]), g0[6:]]), 1.0)):
            _, c = _run_norm(nb, g, 1.0, ncoef=ncoef)
            assert float(c[1]) == flag
            assert abs(float(c[0]) - (rc if flag == 0 else 0.0)) <= tc
            if ncoef >= 4:
                assert c[2:4].tolist() == [1.0, flag]      # the optimizer's (scale, skip) pair
                assert c[4:].tolist() == [SENT] * (ncoef - 4)
            else:
                assert c[2:].tolist() == [SENT] * (ncoef - 2)
    gb, g = _carve(g0)
    nbuf, nrm = _carve(torch.zeros(1, device=DEV))
    cb, c = _carve(torch.full((1,), SENT, device=DEV))
    with pytest.raises(RuntimeError, match="coef_out"):
        nb.grad_norm(g, 1.0, nrm, c)
    torch.cuda.synchronize()
    assert _intact(cb, c) and float(c[0]) == SENT and _intact(gb, g)


# ------------------------------------------------------------------ scale_, fill_, add_i64_
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_scale_is_the_fp32_product(nb, shift):
    for n in NS + [N2S]:
        x0 = _state(n)[4]   # with 0, 1e-30 (a product below the normal range for the small coefficient) and 1e15
        for coef in (0.37, 0.5, 1e-10):
            xb, x = _carve(x0, shift)
            cb, c = _carve(torch.tensor([coef, float("nan"), 3.0], device=DEV))   # only coef[0] is read
            nb.scale_(x, c[:2])
            torch.cuda.synchronize()
            assert _intact(xb, x) and _intact(cb, c)
            assert _biteq(x, _prod32(x0, float(c[0]))), (n, coef)


@pytest.mark.parametrize("value", [float("nan"), -0.0, float("inf"), 1.5])
def test_fill(nb, value):
    for n in NS + [N2V]:
        xb, x = _carve(torch.full((n,), 3.0, device=DEV))
        nb.fill_(x, value)
        torch.cuda.synchronize()
        assert _intact(xb, x)
        if math.isnan(value):
            assert bool(x.isnan().all()), n
        else:
            assert _biteq(x, torch.full((n,), value, device=DEV)), n


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_fill_refuses_a_misaligned_view(nb, shift):
    for n in (1, 5, 1025):
        xb, x = _carve(torch.full((n,), 3.0, device=DEV), shift)
        with pytest.raises(RuntimeError):
            nb.fill_(x, 1.0)
        torch.cuda.synchronize()
        assert _intact(xb, x) and bool((x == 3.0).all())


@pytest.mark.parametrize("addend", [3, -(2 ** 40 + 1), 2 ** 62])
def test_add_i64(nb, addend):
    for n in NS + [N2S]:
        x0 = (2 ** 53 + 1) + 2 * torch.arange(n, dtype=torch.int64, device=DEV)   # odd and above 2^53: no double holds them
        if addend > 2 ** 60:
            x0 = x0 - 2 ** 54   # stays inside int64
        xb, x = _carve(x0, 1, sent=ISENT)
        nb.add_i64_(x, addend)
        torch.cuda.synchronize()
        assert _intact(xb, x, ISENT)
        assert torch.equal(x, x0 + addend) and x.dtype == torch.int64, n


# ------------------------------------------------------------------ gather_
def _gather_case(dtype, n, tail=5):
    g = _gen("gather", n, str(dtype))
    src = torch.randn(37, generator=g, device=DEV).to(dtype)
    src[3] = float("nan") if dtype == F32 else 7.0
    idx = torch.randint(0, 37, (n,), generator=g, device=DEV)   # repeats: 37 sources
    idx[torch.rand(n, generator=g, device=DEV) < 0.3] = -1
    idx[::5] = -5
    if n > 3:
        idx[1] = idx[2] = 36
    dst0 = torch.randn(n + tail, generator=g, device=DEV).to(dtype)
    return src, idx, dst0


def _same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_gather(nb, dtype):
    for n in (1, 7, 257, 1025, N2S):
        src, idx, dst0 = _gather_case(dtype, n)
        db, dst = _carve(dst0)
        sb, s = _carve(src)
        ib, i = _carve(idx, sent=ISENT)
        nb.gather_(dst, s, i)
        torch.cuda.synchronize()
        assert _intact(db, dst) and _intact(sb, s) and _intact(ib, i, ISENT)
        want = R.gather(dst0, src, idx)
        assert _same(dst.float(), want.float()), n
        assert _biteq(dst[n:], dst0[n:])                          # idx shorter than dst: the tail stays
        assert bool((dst[:n][idx < 0] == 0).all())


def test_gather_accumulate(nb):
    for n in (1, 7, 257, 1025, N2S):
        src, idx, dst0 = _gather_case(F32, n)
        db, dst = _carve(dst0)
        sb, s = _carve(src)
        nb.gather_(dst, s, idx, True)
        torch.cuda.synchronize()
        assert _intact(db, dst) and _intact(sb, s) and _biteq(s, src)
        assert _same(dst, R.gather(dst0, src, idx, True)), n      # one fp32 addition per element: exact
        assert _biteq(dst[n:], dst0[n:])
        assert torch.equal(dst[:n][idx < 0], dst0[:n][idx < 0])   # a negative index adds nothing


def test_gather_bf16_accumulate_is_refused(nb):
    src, idx, dst0 = _gather_case(BF16, 257)
    db, dst = _carve(dst0)
    with pytest.raises(RuntimeError):
        nb.gather_(dst, src, idx, True)
    torch.cuda.synchronize()
    assert _intact(db, dst) and _biteq(dst, dst0)


# ------------------------------------------------------------------ cast_weights
def _f32_from_bits(words):
    return torch.tensor(words, dtype=torch.int64).to(torch.int32).view(F32)


# +-0, +-inf, NaN, fp32 denormals, a bf16 denormal and a tie between two of them, exact bf16 ties after an even and
# an odd kept bit (both signs), the largest finite bf16, the same plus half an ulp (-> inf) and just below that
CAST_SPECIAL = _f32_from_bits([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x00000001, 0x807fffff,
                               0x00010000, 0x00018000, 0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x7f7f0000,
                               0x7f7f8000, 0x7f7f7fff, 0xff7f8000, 0x3f808001, 0x3f807fff])


def _source(need, shift, tag):
    """fp32 source view of `need` elements, `shift` floats off 16-byte alignment: randn with the special values
    spread through it (every 3rd element)."""
    buf = torch.randn(need + shift + 4, generator=_gen("castsrc", tag), device=DEV)
    v = buf[shift:shift + need]
    k = v[::3].numel()
    v[::3] = CAST_SPECIAL.to(DEV).repeat(-(-k // len(CAST_SPECIAL)))[:k]
    assert v.data_ptr() % 16 == 4 * (shift % 4)
    return v


def _entry(dims, valid=None, order=(0, 1, 2, 3), shift=0, align=8, odd=0):
    """A cast entry without its offset: the source holds [valid] stored with the destination dims nested in
    `order` (outermost first); align / odd place the destination (elements: a multiple of `align`, plus `odd`)."""
    valid = list(dims) if valid is None else list(valid)
    st, run = [0, 0, 0, 0], 1
    for k in reversed(order):
        st[k] = run
        run *= valid[k]
    return {"dims": list(dims), "valid": valid, "st": st, "need": run, "shift": shift, "align": align, "odd": odd}


T_ORDER = (3, 1, 2, 0)   # source unit stride on destination dim 0: the transpose path when D0, D3 >= 16


def _cast_entries():
    E = []
    # transpose path: every D0 x D3 edge x (D1 D2 in {1, 9}); tiles of 64 x 64, ragged in both directions
    for D0, D3, (D1, D2) in itertools.product((16, 63, 64, 65, 130), (16, 17, 64, 65, 72), ((1, 1), (3, 3))):
        E.append(_entry([D0, D1, D2, D3], order=T_ORDER))
    E.append(_entry([65, 3, 3, 65], valid=[60, 3, 3, 65], order=T_ORDER))    # 36 tiles on 10 blocks; short in dim 0
    E.append(_entry([64, 3, 3, 72], valid=[64, 3, 3, 67], order=T_ORDER))    # short in dim 3
    E.append(_entry([130, 1, 1, 65], valid=[100, 1, 1, 33], order=T_ORDER))  # short in both, whole tiles of padding
    E.append(_entry([64, 3, 3, 64], valid=[63, 2, 1, 61], order=T_ORDER))    # and in dims 1, 2
    for D0, D3 in ((15, 64), (15, 16), (64, 15), (16, 15), (15, 15)):        # below 16: the direct paths
        E.append(_entry([D0, 3, 3, D3], order=T_ORDER))
    E.append(_entry([64, 1, 1, 64], order=T_ORDER, odd=1))                   # the path stores elementwise: any offset
    # identity path and its fall-throughs
    E.append(_entry([1, 1, 1, 8]))                        # n = 8
    E.append(_entry([29, 53, 1, 8]))                      # n = 3 * 4096 + 8: more than one block, ragged
    E.append(_entry([1, 1, 3, 4]))                        # n = 12: n % 8 != 0 -> 4-wide
    E.append(_entry([29, 53, 1, 8], shift=1))             # source one float off -> 4-wide
    E.append(_entry([2, 3, 4, 8], align=8, odd=4))        # destination 8- but not 16-byte aligned (bf16) -> 4-wide
    E.append(_entry([2, 3, 4, 8], odd=1))                 # odd destination offset -> scalar loop
    E.append(_entry([2, 3, 4, 8], odd=2))
    # 4-wide direct path: D3 % 4 == 0, the valid[3] edge inside a quad
    for D3 in (8, 12):
        for v3 in (D3, D3 - 1, D3 - 3, 1):
            E.append(_entry([5, 3, 2, D3], valid=[4, 3, 2, v3]))
            E.append(_entry([5, 3, 2, D3], valid=[5, 2, 1, v3], order=(3, 0, 1, 2)))   # st[3] != 1
    E.append(_entry([20, 3, 3, 16], valid=[17, 3, 2, 13], order=(2, 3, 0, 1)))
    E.append(_entry([5, 3, 2, 8], valid=[5, 3, 2, 8], order=(0, 1, 2, 3), shift=2))
    # scalar loop: D3 % 4 != 0
    for D3 in (1, 3, 5, 7):
        E.append(_entry([6, 2, 3, D3]))
        E.append(_entry([6, 2, 3, D3], valid=[5, 2, 2, max(1, D3 - 2)], order=(1, 0, 3, 2)))
    # more than 1024 * 4096 elements: the entry's 1024 blocks go round its loop twice (4-wide path, padded rows)
    E.append(_entry([1025, 1, 64, 64], valid=[1025, 1, 64, 63]))
    E.append(_entry([3, 1, 1, 4], odd=3))                 # the last entry: the space after it must survive too
    return E


def _run_cast(be, specs):
    """Lay the entries out with sentinel gaps, run ONE launch, compare every entry and every gap."""
    dt = be.act_dtype
    off, entries, metas = 5 * 8, [], []
    for k, e in enumerate(specs):
        n = math.prod(e["dims"])
        off = -(-off // e["align"]) * e["align"] + e["odd"]
        src = _source(e["need"], e["shift"], k)
        entries.append((src, off, e["dims"], e["valid"], e["st"]))
        metas.append((src.clone(), off, n))
        off += n + 3   # a gap before the next one
    total = off + 64
    flat = torch.full((total,), SENT, dtype=dt, device=DEV)
    assert flat.data_ptr() % 32 == 0
    be.cast_weights(entries, total, flat)
    torch.cuda.synchronize()
    covered = torch.zeros(total, dtype=torch.bool, device=DEV)
    for k, ((src, doff, dims, valid, st), (src0, _, n)) in enumerate(zip(entries, metas)):
        assert _biteq(src, src0), k
        ref = R.relayout(src, dims, valid, st).reshape(-1)
        got = flat[doff:doff + n]
        covered[doff:doff + n] = True
        nan = ref.isnan()
        if dt == F32:
            same = _bits(got) == _bits(ref)
            gnan = got.isnan()
        else:
            same = (_bits(got).to(torch.int32) & 0xffff) == R.bf16_bits(ref)
            gnan = got.float().isnan()
        bad = ~torch.where(nan, gnan, same)
        assert not bool(bad.any()), (f"entry {k} dims={dims} valid={valid} st={st} doff={doff}: {int(bad.sum())} of {n} "
                                     f"differ, first at {int(bad.nonzero()[0])}")
    assert bool((flat[~covered] == SENT).all()), "a gap between entries (or the space after the last) was written"
    return len(entries)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_cast_weights_every_branch(nb, nb32, prec):
    specs = _cast_entries()
    assert _run_cast(nb if prec == "bf16" else nb32, specs) >= 20


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_cast_weights_single_entries(nb, nb32, prec):
    """One entry per launch (block map of a single entry), the small ones of each path."""
    be = nb if prec == "bf16" else nb32
    for e in (_entry([65, 3, 3, 65], valid=[60, 3, 3, 65], order=T_ORDER), _entry([1, 1, 1, 8]),
              _entry([5, 3, 2, 8], valid=[4, 3, 2, 5]), _entry([6, 2, 3, 5], valid=[5, 2, 2, 3], order=(1, 0, 3, 2)),
              _entry([2, 3, 4, 8], odd=4), _entry([2, 3, 4, 8], odd=1)):
        _run_cast(be, [e])
