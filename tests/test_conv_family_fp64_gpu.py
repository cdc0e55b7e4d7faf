"""The convolution kernels (conv_igemm.hip, the streaming kernels, head.hip, conv_wgrad.hip,
conv_wgrad3.hip) against the fp64 reference of tests/conv_ref.py at the edge shapes of each path.

Every case
* asserts the path it ran (conv2d_fwd_plan, the *_last flags, the statistics rows returned);
* passes every operand as a column slice of its own wider buffer with NaN around the inputs and a
  sentinel around (and one row after) the outputs, and checks the sentinel afterwards -- the ``dense``
  variants take the aligned / vector-store branches instead;
* compares elementwise with bounds that count roundings (profiles/conv_tests/README.md derives each
  count; u = 2^-24):

    |out - ref| <= h + k u mag     mag = the sum of the absolute terms of the element (conv_ref),
                                   h = half a bf16 ulp at |ref| + k u mag (0 for fp32 storage),
                                   k = (terms - 1) + (split-K slices - 1) + epilogue operations;
    statistics: the rows are added in fp64 and held to (L + r) u sum|term| per channel against fp64
    sums of the kernel's own STORED output, L = the longest fp32 chain (or, where the reduction's
    code was not modelled, the rows one partial covers: a sum of n terms in any order has n - 1
    roundings), r = 1 when the term is a product.
"""
import math

import pytest
import torch

import conv_ref as R
import test_conv_args_cpu as ARGS
from deeplearning_mpi_amd._ext import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 640.0          # exact in bf16; no output below comes near it
NAN = float("nan")

DEFAULTS = dict(set_conv_splitk=0, set_conv_pipe=-1, set_conv_pipe_dgrad=-1, set_conv_halo=-1, set_halo_pipe=1,
                set_dgs_blocks=0, set_dgrad_stream=-1, set_wgrad3=-1, set_wgrad3_blocks=0, set_wgrad_blocks=0,
                set_conv_stream=-1, set_conv3_stream=-1)


@pytest.fixture(scope="module")
def C():
    return native()


@pytest.fixture
def sw(C):
    """sw(name, value) sets a library switch; every switch touched is put back after the test."""
    used = []

    def set_(name, val):
        assert name in DEFAULTS
        used.append(name)
        getattr(C, name)(val)

    yield set_
    for name in used:
        getattr(C, name)(DEFAULTS[name])


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """A HIP error is sticky: nothing more is launched in this process once one is seen."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, stopping: {e}", returncode=3)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


class Op:
    """A [rows, C] operand as a column slice [off, off + C) of its own [rows (+1), ld] buffer."""

    def __init__(self, rows, Cc, dtype, fill, ld=None, off=0, extra_row=False):
        self.rows, self.C, self.off = rows, Cc, off
        self.ld = Cc if ld is None else ld
        assert 0 <= off and off + Cc <= self.ld
        self.fill = fill
        self.buf = torch.full((rows + (1 if extra_row else 0), self.ld), fill, device=DEV, dtype=dtype)

    @property
    def v(self):
        return self.buf[:self.rows, self.off:self.off + self.C]

    def untouched_outside(self):
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        keep[:self.rows, self.off:self.off + self.C] = False
        return bool((self.buf[keep] == self.fill).all())


def _input(g, rows, Cc, dtype, pad, off, scale=1.0, values=None):
    """An input slice: NaN outside.  pad = 0: dense."""
    op = Op(rows, Cc, dtype, NAN, Cc + pad, off if pad else 0)
    op.v.copy_((_randn(g, rows, Cc, scale=scale) if values is None else values).to(dtype))
    return op


def _output(rows, Cc, dtype, pad, off, ld=None):
    return Op(rows, Cc, dtype, SENT, (Cc + pad) if ld is None else ld, off if (pad or ld) else 0, extra_row=True)


def _le(err, tol):
    return bool((err <= tol).all())


def _worst(err, tol):
    r = torch.nan_to_num(err / tol.clamp_min(1e-300), nan=float("inf"))
    return f"worst err / bound = {r.max().item():.3g} at {tuple(int(i) for i in (r == r.max()).nonzero()[0])}"


def check_elem(out, ref, mag, k, what):
    """|out - ref| <= h + k u mag, h taken at |ref| + k u mag."""
    slack = k * U * mag
    tol = R.store_tol(ref.abs() + slack, out.dtype) + slack
    err = (out.double() - ref).abs()
    kmax = k.max().item() if torch.is_tensor(k) else k
    print(f"{what}: {_worst(err, tol)} (k = {kmax:g})")
    assert _le(err, tol), f"{what}: {_worst(err, tol)} (k = {kmax:g})"


def check_partials(part, rows, refs, L, what):
    """part [rows + 1][len(refs)][C] fp32 partial rows (the last one a NaN sentinel) against
    refs = [(sum, sum of |term|, r)] per statistic."""
    assert part.shape[0] == rows + 1 and bool(part[rows].isnan().all()), f"{what}: the row after the partials was written"
    assert bool(torch.isfinite(part[:rows]).all()), f"{what}: a partial row was not written"
    got = part[:rows].double().sum(0)
    for i, (ref, absref, r) in enumerate(refs):
        err, tol = (got[i] - ref).abs(), (L + r) * U * absref
        print(f"{what} statistic {i}: {_worst(err, tol)} (L = {L})")
        assert _le(err, tol), f"{what} statistic {i}: {_worst(err, tol)} (L = {L})"


def epilogue_chain(bm, bn, threads=256):
    """conv_epilogue: a thread walks ceil(bm / RG) rows (+ up to one per pass, <= 8 passes), then RG
    partials are added; RG = threads / (bn / 8)."""
    rg = threads // (bn // 8)
    return math.ceil(bm / rg) + 8 + rg


def splitk_roundings(tiles, maxk, forced):
    """Additions of split-K slices: conv_igemm.hip splitk_plan (tiles x slices towards 256 blocks, >= 4
    K-steps a slice, <= 8 slices) or the forced count, capped at the K-steps; S slices are summed from
    zero: S - 1 roundings."""
    if forced > 0:
        S = forced
    elif tiles >= 256 or maxk < 8:
        S = 1
    else:
        S = min(math.ceil(256 / tiles), maxk // 4, 8)
        S = 1 if S < 2 else S
    if S > maxk:
        S = maxk if maxk > 0 else 1
    return S - 1


def halo_tiles_per_image(P, Q, bm):
    """conv_plan.cpp halo_geom: the th x tw tile (th * tw <= bm, halo rows <= 352 / 192) with the fewest tiles."""
    best, rows = None, 352 if bm == 256 else 192
    for w in range(32 if bm == 256 else 16, 3, -1):
        h = min(bm // w, rows // (w + 2) - 2)
        if h >= 1:
            t = math.ceil(P / h) * math.ceil(Q / w)
            best = t if best is None or t < best else best
    return best


# ====================================================================== forward
def run_fwd(C, N, H, W, Ci, K, geo, *, path, dtype=BF16, ydtype=None, bias=True, stats=False, affine=False, res=False,
            relu=False, kvalid=0, bm=0, bn=0, sliced=True, ldy=None, yoff=None, splitk=0, seed=0, expect_tile=None):
    """splitk: the count forced with set_conv_splitk (0: the rule)."""
    g = _gen(seed * 7919 + N * 131 + H * 17 + W + Ci + K)
    geo = R.Geo(*geo)
    ydtype = ydtype or dtype
    f32 = int(dtype == F32)
    P, Q = R.out_hw(H, W, geo)
    M, n = N * P * Q, geo.R * geo.S * Ci
    stored = kvalid if 0 < kvalid < K else K
    x = _input(g, N * H * W, Ci, dtype, 24 if sliced else 0, 8)
    w = _randn(g, K, geo.R, geo.S, Ci, scale=n ** -0.5).to(dtype)
    y = _output(M, stored, ydtype, 40 if sliced else 0, 16, ld=ldy) if yoff is None else \
        Op(M, stored, ydtype, SENT, ldy, yoff, extra_row=True)
    b = _randn(g, K) if bias else None
    sc, sh = (_randn(g, K) + 1.5, _randn(g, K)) if affine else (None, None)
    r = _input(g, M, K, dtype, 8 if sliced else 0, 8) if res else None
    plan = C.conv2d_fwd_plan(N, H, W, Ci, K, geo.R, geo.S, geo.stride, geo.pad, 0, f32, bm, bn, res, affine, relu,
                             stats, False, kvalid, x.ld, x.off, y.ld, y.off)
    assert plan["path"] == path, plan
    if expect_tile:
        assert (plan["bm"], plan["bn"]) == expect_tile, plan
    rows = plan["rows"]
    st = torch.full((rows + 1, 2, K), NAN, device=DEV) if stats else None
    got_rows = C.conv2d_fwd(x.buf, N, H, W, Ci, x.ld, x.off, w, K, geo.R, geo.S, geo.stride, geo.pad, y.buf, y.ld, y.off,
                            b, r.buf if res else None, r.ld if res else 0, r.off if res else 0, sc, sh, relu, st, bm,
                            kvalid, bn)
    torch.cuda.synchronize()
    assert got_rows == (0 if path == "head" else rows)
    flags = dict(halo=C.conv_halo_last(), stream1x1=C.conv_stream_last(), stream3x3=C.conv3_stream_last(),
                 head=C.head1x1_last(), c8=C.conv_c8_last(), c16=C.conv_c16_last())
    for name, ran in flags.items():
        if name == "halo" and path not in ("halo", "pipe", "igemm"):
            continue   # (the flag belongs to the tiled launches)
        assert ran == int(name == path), (path, flags)
    what = f"fwd {path} {N}x{H}x{W} {Ci}->{K} {tuple(geo)} tile {plan['bm']}x{plan['bn']}"
    assert y.untouched_outside(), f"{what}: wrote outside its slice, past M or past kvalid"
    ref, mag, _ = R.fwd(x.v.reshape(N, H, W, Ci), w, geo, b, sc, sh, r.v.reshape(N, P, Q, K) if res else None, relu)
    terms = n if not f32 else 2 * n     # fp32 x fp32 products round; bf16 x bf16 are exact in fp32
    nsplit = 0
    if path in ("igemm", "halo"):       # (the pipelined and persistent kernels never split)
        nsplit = splitk_roundings(rows * math.ceil(K / plan["bn"]), math.ceil(n / (32 if f32 else 64)), splitk)
    k = (terms - 1) + nsplit + int(bias) + 2 * int(affine) + int(res)
    check_elem(y.v, ref.reshape(M, K)[:, :stored], mag.reshape(M, K)[:, :stored], k, what)
    if stats:
        assert stored == K and not (affine or res or relu) and ydtype == dtype
        (s1, s2), (a1, a2) = R.stats(y.v)
        if path == "stream3x3":    # 2 fragment rows per tile and trip, then WGM * 16 = 64 partials
            L = 2 * math.ceil(N * math.ceil(H / plan["th"]) * math.ceil(W / plan["tw"]) / plan["G"]) + 64
        elif path == "stream1x1":  # BM / RG rows per trip, then RG partials
            rg = 2048 // plan["sbn"]
            L = (plan["sbm"] // rg) * math.ceil(math.ceil(M / plan["sbm"]) / plan["G"]) + rg
        elif path in ("c8", "c16"):  # GP groups per wave and pass, then 4 shuffles and the 4 waves
            gp = 2 if path == "c8" else 1
            L = gp * math.ceil(math.ceil(M / 16) / (plan["G"] * 4 * gp)) + 7
        else:
            L = epilogue_chain(plan["bm"], plan["bn"], 512 if path == "pipe" else 256)
        check_partials(st, rows, [(s1, a1, 0), (s2, a2, 1)], L, what + " stats")
    return plan


G3 = (3, 3, 1, 1)
G3S2 = (3, 3, 2, 1)
G1 = (1, 1, 1, 0)
G1S2 = (1, 1, 2, 0)
G7 = (7, 7, 2, 3)
TILES = [(64, 64), (64, 128), (128, 64), (128, 128), (256, 64), (256, 128)]


@pytest.mark.parametrize("bm,bn", TILES, ids=[f"{a}x{b}" for a, b in TILES])
def test_igemm_tiles(C, bm, bn):
    """A: every single-stage tile with small-channel (C = 8, 16, 32) and regular (64, 128) staging, the
    five geometries, row and column remainders, each epilogue, bf16 and fp32 output."""
    kw = dict(path="igemm", bm=bm, bn=bn, expect_tile=(bm, bn))
    run_fwd(C, 3, 9, 11, 64, 192, G3, stats=True, **kw)                              # 297 rows: a remainder in every tile
    run_fwd(C, 3, 9, 11, 16, 64, G3S2, affine=True, res=True, relu=True, **kw)
    run_fwd(C, 3, 7, 7, 8, 64, G7, ydtype=F32, **kw)
    run_fwd(C, 3, 7, 7, 128, 128, G1, stats=True, **kw)
    run_fwd(C, 3, 9, 11, 32, 192, G1S2, ydtype=F32, **kw)
    run_fwd(C, 2, 9, 11, 64, 128, G3, ydtype=F32, affine=True, res=True, relu=True, **kw)   # h = 0: one product of 576 shows
    run_fwd(C, 3, 9, 11, 64, 8, G3, kvalid=3, ldy=11, yoff=5, **kw)                  # scalar stores into an odd ldy
    run_fwd(C, 2, 7, 7, 64, 192, G3, stats=True, sliced=False, **kw)                 # dense
    run_fwd(C, 2, 7, 7, 64, 8, G3, kvalid=3, sliced=False, **kw)                     # dense, ldy = 3


@pytest.mark.parametrize("req", [0, 2, 3, 8, 100])
def test_igemm_splitk(C, sw, req):
    """Split-K by the rule (4x4 grid, 512 -> 512, 3x3: 8 slices of 72 K-steps) and forced, a request
    larger than the 9 K-steps included."""
    if req == 0:
        run_fwd(C, 1, 4, 4, 512, 512, G3, path="igemm", stats=True)
        return
    sw("set_conv_splitk", req)
    run_fwd(C, 3, 9, 11, 64, 192, G3, path="igemm", bm=64, bn=64, stats=True, splitk=req)
    run_fwd(C, 3, 9, 11, 16, 64, G3S2, path="igemm", bm=128, bn=64, ydtype=F32, res=True, splitk=req)


F32_TILES = [(64, 64), (64, 128), (128, 64), (128, 128)]


@pytest.mark.parametrize("bm,bn", F32_TILES, ids=[f"{a}x{b}" for a, b in F32_TILES])
def test_f32_tiles(C, bm, bn):
    """B: fp32 activations on the four launch_f32 tiles, small (C = 8, 48) and regular (32, 64) staging."""
    kw = dict(path="igemm", dtype=F32, bm=bm, bn=bn, expect_tile=(bm, bn))
    run_fwd(C, 3, 9, 11, 8, 192, G3, stats=True, **kw)
    run_fwd(C, 3, 9, 11, 48, 64, G1, affine=True, res=True, relu=True, **kw)
    run_fwd(C, 3, 9, 11, 32, 192, G3, res=True, **kw)
    run_fwd(C, 3, 7, 7, 64, 128, G1, stats=True, sliced=False, **kw)


PIPE = [(64, 256, 0, 0, (256, 256)), (64, 256, 128, 256, (128, 256)), (64, 128, 0, 0, (256, 128)),
        (128, 64, 0, 0, (512, 64))]


@pytest.mark.parametrize("Ci,K,bm,bn,tile", PIPE, ids=[f"{t[0]}x{t[1]}" for *_, t in PIPE])
def test_pipe_tiles(C, sw, Ci, K, bm, bn, tile):
    """C: the pipelined 8-wave tiles, 297 rows (a remainder in each)."""
    if not bn:
        sw("set_conv_pipe", 1)
    for sliced in (True, False):
        run_fwd(C, 3, 9, 11, Ci, K, G3, path="pipe", stats=True, bm=bm, bn=bn, expect_tile=tile, sliced=sliced)
    run_fwd(C, 3, 9, 11, Ci, K, G3, path="pipe", bm=bm, bn=bn, expect_tile=tile, affine=True, res=True, relu=True)


def test_pipe_224_by_the_rule(C):
    """pipe_select takes 224 x 256 where ceil(M / 128) > 256 >= ceil(M / 224): 2 x 130 x 131, 3x3 pad 0,
    128 -> 256 (33,024 rows: 258 / 148 tiles)."""
    run_fwd(C, 2, 130, 131, 128, 256, (3, 3, 1, 0), path="pipe", stats=True, expect_tile=(224, 256))


# The tile rules (conv_plan.cpp pick_tiles / halo_tiles) give every grid below 8,192 rows 64-wide columns
# and with them the 256 x 64 halo tile; the 128 x 128 and 256 x 128 halo tiles are reached from 16,384
# rows (K = 128) and 8,192 rows (K = 256) only: the smallest such odd grids stand for them.
HALO = [(64, [(3, 9, 11), (3, 1, 1), (2, 17, 5)], (256, 64)), (128, [(1, 129, 128)], (128, 128)),
        (256, [(1, 91, 91)], (256, 128))]


@pytest.mark.parametrize("K,grids,tile", HALO, ids=[f"{t[0]}x{t[1]}" for *_, t in HALO])
@pytest.mark.parametrize("halo_pipe", [1, 0])
def test_halo_tiles(C, sw, K, grids, tile, halo_pipe):
    """D: halo tiles on grids that leave partial tiles in both directions, both halo-pipe settings,
    forced split-K (the 256 x 128 tile then runs single-stage)."""
    sw("set_conv_halo", 2)
    sw("set_halo_pipe", halo_pipe)
    for (N, H, W) in grids:
        run_fwd(C, N, H, W, 128, K, G3, path="halo", stats=True, expect_tile=tile)
    N, H, W = grids[0]
    run_fwd(C, N, H, W, 128, K, G3, path="halo", affine=True, res=True, relu=True, sliced=False, expect_tile=tile)
    sw("set_conv_splitk", 3)
    run_fwd(C, N, H, W, 128, K, G3, path="halo", stats=True, expect_tile=tile, splitk=3)


@pytest.mark.parametrize("H,W", [(28, 28), (29, 31)])
def test_halo_by_the_rule(C, H, W):
    run_fwd(C, 1, H, W, 64, 128, G3, path="halo", stats=True, expect_tile=(256, 64))


@pytest.mark.parametrize("N,H,W", [(3, 9, 11), (3, 1, 1), (3, 17, 5)])
@pytest.mark.parametrize("stats", [True, False])
def test_stream3x3(C, sw, N, H, W, stats):
    """E: the persistent 64 -> 64 3x3 kernel; 3 tiles on 2 blocks: a second trip the grid does not divide."""
    sw("set_dgs_blocks", 2)
    plan = run_fwd(C, N, H, W, 64, 64, G3, path="stream3x3", stats=stats)
    tiles = N * math.ceil(H / plan["th"]) * math.ceil(W / plan["tw"])
    assert plan["G"] == 2 and tiles > plan["G"] and tiles % plan["G"] != 0
    run_fwd(C, 1, H, W, 64, 64, G3, path="stream3x3", stats=stats, sliced=False)


# (C, K, stride, N, H, W): M = N*P*Q rows chosen so that the M-tiles exceed the plan's G and the last
# tile holds one row
STREAM1 = [(64, 64, 1, 1, 115, 571), (64, 2048, 1, 1, 17, 241), (128, 2048, 1, 1, 3, 683), (256, 2048, 1, 1, 25, 41),
           (256, 2048, 2, 1, 49, 81)]


@pytest.mark.parametrize("Ci,K,stride,N,H,W", STREAM1, ids=[f"{c}-{k}-s{s}" for c, k, s, *_ in STREAM1])
def test_stream1x1(C, Ci, K, stride, N, H, W):
    geo = (1, 1, stride, 0)
    plan = run_fwd(C, N, H, W, Ci, K, geo, path="stream1x1", stats=True)
    P, Q = R.out_hw(H, W, R.Geo(*geo))
    M = N * P * Q
    assert math.ceil(M / plan["sbm"]) > plan["G"], plan          # a second trip
    assert M % plan["sbm"] == 1, (M, plan)                       # a last tile of one row
    run_fwd(C, 1, 9, 11, Ci, K if K == 64 else 128, geo, path="stream1x1", stats=False, sliced=False)


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("W", [16, 32])
def test_c8(C, H, W):
    """E: the 8-channel 3x3 kernel.  A block's 4 waves take 8 pixel groups per pass and the grid holds
    one block per 16 groups, so 3 x 5 x 32 (30 groups, 2 blocks) runs the loop twice."""
    for N in (1, 3):
        plan = run_fwd(C, N, H, W, 8, 64, G3, path="c8", stats=True)
        assert plan["G"] == max(1, math.ceil(math.ceil(N * H * W / 16) / 16))
    run_fwd(C, 2, H, W, 8, 64, G3, path="c8", sliced=False)


@pytest.mark.parametrize("H", [4, 6])
@pytest.mark.parametrize("W", [19, 35])
def test_c16(C, H, W):
    """E: the 16-channel 4x4 stem kernel (4 groups per pass: 3 x 3 x 32 outputs = 18 groups on 2 blocks
    run three passes)."""
    for N in (1, 3):
        run_fwd(C, N, H, W, 16, 64, (4, 4, 1, 0), path="c16", stats=True)
    run_fwd(C, 2, H, W, 16, 64, (4, 4, 1, 0), path="c16", sliced=False)


@pytest.mark.parametrize("Ci", [16, 512])
@pytest.mark.parametrize("kv", [1, 4])
@pytest.mark.parametrize("ydtype", [BF16, F32], ids=["bf16", "fp32"])
def test_head(C, Ci, kv, ydtype):
    """E: the 1x1 head, one row and more rows than a block covers (16 * 64 / (C / 8))."""
    for (N, H, W) in ((1, 1, 1), (1, 23, 29)):
        run_fwd(C, N, H, W, Ci, 8, G1, path="head", kvalid=kv, ydtype=ydtype, ldy=kv + 7, yoff=3)
    run_fwd(C, 1, 5, 7, Ci, 8, G1, path="head", kvalid=kv, ydtype=ydtype, sliced=False)


# ====================================================================== data gradient
def _bits(mask):
    rows, Cc = mask.shape
    w = 2 ** torch.arange(8, device=DEV, dtype=torch.int32)
    return (mask.reshape(rows, Cc // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).contiguous()


def run_dgrad(C, N, H, W, K, Cc, geo, *, path, dtype=BF16, res=False, bias=False, colsum=False, mode=None, z2=False,
              sliced=True, splitk=0, seed=0, tile=None, pipe=False):
    """dx [N*H*W, Cc] from dy [N*P*Q, K]; mode: None | mask | two | from_z | bits.  tile: the (bm, bn) the
    rules give this shape (igemm: 64 x 64, halo: 256 x 64 unless said) -- asserted through the rows of the
    partials wherever the launch returns any; pipe: the tile is a pipelined one; splitk: the forced count."""
    g = _gen(seed * 104729 + N * 131 + H * 17 + W + K + Cc)
    geo = R.Geo(*geo)
    P, Q = R.out_hw(H, W, geo)
    Min, M, n = N * H * W, N * P * Q, geo.R * geo.S * K
    pad = 24 if sliced else 0
    dy = _input(g, M, K, dtype, pad, 8)
    wT = _randn(g, Cc, geo.R, geo.S, K, scale=n ** -0.5).to(dtype)
    dx = _output(Min, Cc, dtype, 40 if sliced else 0, 16)
    r = _input(g, Min, Cc, dtype, 8 if sliced else 0, 8) if res else None
    b = _randn(g, Cc) if bias else None
    none = (None, 0, 0)
    t = lambda op: (op.buf, op.ld, op.off) if op is not None else none   # noqa: E731
    mask = z = zz2 = msc = msh = mb = None
    if mode is not None:
        z = _input(g, Min, Cc, dtype, 16 if sliced else 0, 8)
        if mode in ("mask", "two"):     # a stored ReLU output: positive, zero and negative values
            vals = _randn(g, Min, Cc)
            vals[torch.rand(Min, Cc, generator=g, device=DEV) < 0.4] = 0.0
            mask = _input(g, Min, Cc, dtype, 8 if sliced else 0, 8, values=vals)
        if mode == "two" or z2:
            zz2 = _input(g, Min, Cc, dtype, 24 if sliced else 0, 16)
        if mode == "from_z":
            msc = (torch.rand(Cc, generator=g, device=DEV) + 0.5) * (torch.randint(0, 2, (Cc,), generator=g, device=DEV) * 2 - 1)
            msh = _randn(g, Cc)
        if mode == "bits":
            mb = _bits(torch.rand(Min, Cc, generator=g, device=DEV) < 0.6)
    part = C.conv2d_dgrad_pro(dy.buf, N, P, Q, K, dy.ld, dy.off, wT, Cc, geo.R, geo.S, geo.stride, geo.pad, H, W,
                              dx.buf, dx.ld, dx.off, *t(r), *t(mask), *t(z), *t(zz2), msc, msh, mb, colsum, 0, None,
                              None, None, 0, 0, b)
    torch.cuda.synchronize()
    flags = dict(halo=C.conv_halo_last(), dgrad_stream=C.dgrad_stream_last(), stream3x3=C.conv3_stream_last())
    if path in ("dgrad_stream", "stream3x3"):
        flags.pop("halo")
    for name, ran in flags.items():
        assert ran == int(name == path), (path, flags)
    what = f"dgrad {path} {N}x{H}x{W} {K}->{Cc} {tuple(geo)} mode {mode} tile {tile}"
    assert dx.untouched_outside(), f"{what}: wrote outside its slice or past the last row"

    # the launch's partial rows, its longest statistics chain L and its split-K additions, from the tile
    nsplit = 0
    if path in ("igemm", "halo"):
        bm, bn = tile or ((256, 64) if path == "halo" else (64, 64))
        st, mtiles, maxk = geo.stride, 0, 0
        for ph in range(st):
            for pw in range(st):
                r0, s0 = (ph + geo.pad) % st, (pw + geo.pad) % st
                taps = (-(-(geo.R - r0) // st) if r0 < geo.R else 0) * (-(-(geo.S - s0) // st) if s0 < geo.S else 0)
                maxk = max(maxk, math.ceil(taps * K / (64 if dtype == BF16 else 32)))
                mtiles += math.ceil(N * ((H - ph + st - 1) // st) * ((W - pw + st - 1) // st) / bm)
        if path == "halo":
            mtiles = N * halo_tiles_per_image(H, W, bm)
        want_rows, L = mtiles, epilogue_chain(bm, bn, 512 if pipe else 256)
        if not pipe:
            nsplit = splitk_roundings(mtiles * math.ceil(Cc / bn), maxk, splitk)
    elif path == "stream3x3":   # the forward kernel with flipped taps: the forward plan's tiles and blocks
        pl = C.conv2d_fwd_plan(N, H, W, 64, 64, 3, 3, 1, 1, 0, 0, 0, 0, False, False, False, True, False, 0, 64, 0, 64, 0)
        assert pl["path"] == "stream3x3"
        want_rows = pl["G"]
        L = 2 * math.ceil(N * math.ceil(H / pl["th"]) * math.ceil(W / pl["tw"]) / pl["G"]) + 64
    else:   # conv1x1_dgrad_stream.hip: its plan's rows per tile, G blocks a column; a lane adds TM
        # fragments per trip, then WGM * 16 partials are added in order
        sbm = 64 if K == 128 else ((32 if z2 or mode == "two" else 48) if K == 256 else
                                   (32 if (res or z2 or mode == "bits") else 64))
        sbn = 64 if K == 512 else 128
        G = min(math.ceil(Min / sbm), max(8, C.dgs_blocks() // (Cc // sbn)))
        wgm = 3 if sbm == 48 else 2
        want_rows, L = G, (sbm // (wgm * 16)) * math.ceil(math.ceil(Min / sbm) / G) + wgm * 16

    ref, mag = R.dgrad(dy.v.reshape(N, P, Q, K), wT, geo, H, W, r.v.reshape(N, H, W, Cc) if res else None, b)
    _, cmag = R.dgrad(dy.v.reshape(N, P, Q, K), wT, geo, H, W)
    ref, mag, cmag = ref.reshape(Min, Cc), mag.reshape(Min, Cc), cmag.reshape(Min, Cc)
    terms = n if dtype == BF16 else 2 * n    # fp32 x fp32 products round
    # a pixel no tap reaches (the empty phases of 1x1 / s2) is res + bias alone: at most 2 roundings
    k = torch.where(cmag == 0, torch.full_like(cmag, int(bias) + int(res)),
                    torch.full_like(cmag, (terms - 1) + nsplit + int(bias) + int(res)))
    out = dx.v
    excluded = 0.0
    if mode is None:
        check_elem(out, ref, mag, k, what)
        if not (res or bias):
            assert bool((out[cmag == 0] == 0).all()), f"{what}: pixels without a tap are not exact zeros"
    else:
        unsure = None
        if mode in ("mask", "two"):
            m = R.relu_mask(y=mask.v)
        elif mode == "bits":
            m = R.relu_mask(bits=mb)
        else:
            m, pre, pmag = R.relu_mask(z=z.v, mscale=msc, mshift=msh)
            unsure = pre.abs() <= 2 * U * pmag      # the fp32 fma (or product and sum) may land on either side
            excluded = unsure.double().mean().item()
            print(f"{what}: undecided mask share {excluded:.2e}")
            assert excluded <= 1e-3, f"{what}: {excluded:.2e} of the mask elements are undecided"
        zero = torch.zeros_like(ref)
        dref, dmag = torch.where(m, ref, zero), torch.where(m, mag, zero)
        if unsure is not None and bool(unsure.any()):
            took = out != 0    # at an undecided element: the output is consistent with the mask the kernel took
            dref = torch.where(unsure, torch.where(took, ref, zero), dref)
            dmag = torch.where(unsure, torch.where(took, mag, zero), dmag)
        check_elem(out, dref, dmag, k, what)
        assert bool((out[~m if unsure is None else (~m & ~unsure)] == 0).all()), f"{what}: masked elements are not zero"
    if mode is not None or colsum:
        assert part is not None
        rows = part.shape[0]
        assert rows == want_rows, f"{what}: {rows} partial rows, {want_rows} expected of this tile"
        if colsum and mode is None:
            (s1, s2), (a1, a2) = R.colsum(out)
            refs = [(s1, a1, 0), (s2, a2, 1)]
        else:
            refs = [(s, a, int(i > 0)) for i, (s, a) in enumerate(R.bnbwd_partials(out, z.v, zz2.v if zz2 is not None else None))]
        assert part.shape[1] == len(refs) and part.shape[2] == Cc
        sent = torch.cat([part, torch.full_like(part[:1], NAN)])   # (the binder allocates the partials itself)
        check_partials(sent, rows, refs, L, what + " partials")
    else:
        assert part is None
    return excluded


@pytest.mark.parametrize("H,W", [(15, 15), (16, 15), (7, 9)])
def test_dgrad_stride2_unequal_phases(C, H, W):
    """F: 3x3 / s2 / p1 on grids whose four sub-pixel phases differ in size."""
    run_dgrad(C, 2, H, W, 64, 64, G3S2, path="igemm")
    run_dgrad(C, 2, H, W, 128, 192, G3S2, path="igemm", res=True, bias=True)
    run_dgrad(C, 2, H, W, 64, 64, G3S2, path="igemm", colsum=True, sliced=False)


@pytest.mark.parametrize("splitk", [0, 2])
def test_dgrad_1x1_stride2_empty_phases(C, sw, splitk):
    """1x1 / s2 on 13 x 14: three phases have no tap (zero K-steps); their rows are res + bias (held to
    those two roundings), or exact zeros -- also with the K loop split."""
    if splitk:
        sw("set_conv_splitk", splitk)
    run_dgrad(C, 2, 13, 14, 128, 64, G1S2, path="igemm", splitk=splitk)
    run_dgrad(C, 2, 13, 14, 128, 64, G1S2, path="igemm", res=True, bias=True, splitk=splitk)
    run_dgrad(C, 2, 13, 14, 128, 64, G1S2, path="igemm", res=True, splitk=splitk, sliced=False)
    run_dgrad(C, 2, 13, 14, 128, 64, G1S2, path="igemm", colsum=True, bias=True, splitk=splitk)


def test_dgrad_7x7_and_stride1(C):
    run_dgrad(C, 2, 9, 11, 64, 8, G7, path="igemm", res=True)
    run_dgrad(C, 2, 9, 11, 64, 8, G7, path="igemm", colsum=True, sliced=False)
    run_dgrad(C, 3, 9, 11, 64, 128, G3, path="igemm", bias=True, res=True)
    run_dgrad(C, 3, 9, 11, 128, 64, (3, 3, 1, 0), path="igemm", colsum=True)
    run_dgrad(C, 3, 9, 11, 64, 192, G1, path="igemm", res=True)
    run_dgrad(C, 3, 9, 11, 32, 64, G1, path="igemm", dtype=F32, bias=True, res=True)


# conv2d_dgrad has no tile request: the larger single-stage tiles by the rule (conv_plan.cpp pick_tiles
# on M = N H W / stride^2, Kout = C), each at the smallest odd grid that gives it; the column sums'
# rows (ceil(M / bm) per phase) assert the tile height.  (N, H, W, K, C, geometry, tile)
DGRAD_TILES = [
    (1, 127, 129, 64, 128, G1, (64, 128)),      # 16,383 rows: 128 tiles of 128 (< 512: 64 rows), 256 of 64 (bn stays 128)
    (1, 257, 257, 64, 128, G3S2, (64, 128)),    # four unequal phases of about 16,512 rows
    (1, 257, 255, 64, 128, G1, (128, 128)),     # 65,535 rows: 512 tiles of 128
    (1, 257, 255, 64, 64, G1, (128, 64)),
    (2, 257, 255, 32, 64, G1, (256, 64)),       # cin < 64 and 512 tiles of 256 rows
    (1, 181, 181, 1024, 256, G1, (256, 128)),   # 1x1 from 1024 channels into 256, set_conv_pipe_dgrad(0)
]


@pytest.mark.parametrize("N,H,W,K,Cc,geo,tile", DGRAD_TILES, ids=[f"{t[0]}x{t[1]}-{i}" for i, (*_, t) in enumerate(DGRAD_TILES)])
def test_dgrad_tiles_by_the_rule(C, sw, N, H, W, K, Cc, geo, tile):
    if tile == (256, 128):
        sw("set_conv_pipe_dgrad", 0)
    run_dgrad(C, N, H, W, K, Cc, geo, path="igemm", tile=tile, colsum=True, bias=True)
    run_dgrad(C, N, H, W, K, Cc, geo, path="igemm", tile=tile, mode="mask", res=True, sliced=False)


def test_dgrad_pipe_by_the_rule(C):
    """32,761 rows, 1024 -> 256: pipe_select takes 128 x 256 (256 tiles in one round)."""
    run_dgrad(C, 1, 181, 181, 1024, 256, G1, path="igemm", tile=(128, 256), pipe=True, colsum=True)
    run_dgrad(C, 1, 181, 181, 1024, 256, G1, path="igemm", tile=(128, 256), pipe=True, mode="bits", res=True)


@pytest.mark.parametrize("K,Cc,ptile", [(128, 64, (512, 64)), (128, 128, (256, 128)), (128, 256, (256, 256))])
def test_dgrad_halo_and_pipe(C, sw, K, Cc, ptile):
    """Halo and pipelined data gradients (P == H, Q == W).  The pipelined tiles have no flag of their own:
    the rows of the returned partials tell them (1 or 2 rows of 297 pixels) from the 64-row tile (5 rows),
    which set_conv_pipe_dgrad(0) brings back."""
    sw("set_conv_halo", 2)
    for (N, H, W) in ((3, 9, 11), (2, 17, 5)):
        run_dgrad(C, N, H, W, K, Cc, G3, path="halo", res=True)
        run_dgrad(C, N, H, W, K, Cc, G3, path="halo", colsum=True)
    run_dgrad(C, 3, 9, 11, K, Cc, G3, path="halo", mode="mask", sliced=False)
    sw("set_conv_halo", 0)
    sw("set_conv_pipe", 1)
    run_dgrad(C, 3, 9, 11, K, Cc, G3, path="igemm", tile=ptile, pipe=True, colsum=True, bias=True)
    run_dgrad(C, 3, 9, 11, K, Cc, G3, path="igemm", tile=ptile, pipe=True, mode="two", res=True, bias=True)
    sw("set_conv_pipe_dgrad", 0)
    run_dgrad(C, 3, 9, 11, K, Cc, G3, path="igemm", colsum=True, bias=True)
    run_dgrad(C, 3, 9, 11, K, Cc, G3, path="igemm", mode="two", res=True, bias=True)


@pytest.mark.parametrize("mode", ["mask", "two", "from_z", "bits"])
def test_dgrad_fused_epilogue_igemm(C, mode):
    """The igemm BN-backward epilogue in its four modes on a 1x1 and a 3x3 shape."""
    run_dgrad(C, 3, 9, 11, 64, 64, G1, path="igemm", mode=mode)
    run_dgrad(C, 3, 9, 11, 64, 128, G3, path="igemm", mode=mode, res=(mode != "from_z"))
    run_dgrad(C, 2, 15, 15, 64, 64, G3S2, path="igemm", mode=mode, sliced=False)


@pytest.mark.parametrize("mode", [None, "from_z"])
def test_dgrad_stream3x3(C, sw, mode):
    """The streaming 3x3 kernel with flipped taps: mode 1 (plain) and mode 2 (mask from z), 3 tiles on 2 blocks."""
    sw("set_dgs_blocks", 2)
    for (N, H, W) in ((3, 9, 11), (3, 1, 1), (3, 17, 5)):
        run_dgrad(C, N, H, W, 64, 64, G3, path="stream3x3", mode=mode)
    run_dgrad(C, 1, 9, 11, 64, 64, G3, path="stream3x3", mode=mode, sliced=False)


DGS = [(128, 128), (256, 128), (512, 64)]
DGS_M = 192 * 6 + 1     # 1 (mod 64, 48 and 32): every instance ends with a tile of one row; 19 to 37 tiles


@pytest.mark.parametrize("K,Cc", DGS, ids=[f"K{k}" for k, _ in DGS])
@pytest.mark.parametrize("mode", [None, "bits", "from_z"])
def test_dgrad_stream(C, sw, K, Cc, mode):
    """Every streaming 1x1 data-gradient instance in modes 0 / 1 / 2, with z2 and res where built
    (set_dgrad_stream(2): the opt-in 32-row tiles), on 8 blocks per column so that every block runs 3 to
    5 trips, the last tile holding one row."""
    sw("set_dgrad_stream", 2)
    sw("set_dgs_blocks", 8)
    N, H, W = 1, 1, DGS_M
    if mode is None:
        run_dgrad(C, N, H, W, K, Cc, G1, path="dgrad_stream")
        run_dgrad(C, N, H, W, K, Cc, G1, path="dgrad_stream", res=True, bias=True, sliced=False)
        return
    run_dgrad(C, N, H, W, K, Cc, G1, path="dgrad_stream", mode=mode)
    run_dgrad(C, N, H, W, K, Cc, G1, path="dgrad_stream", mode=mode, res=True, sliced=False)
    run_dgrad(C, N, H, W, K, Cc, G1, path="dgrad_stream", mode=mode, z2=True)


# ====================================================================== weight gradient
def run_wgrad(C, N, H, W, Cc, Ko, geo, *, dtype=BF16, Creal=None, Ko_real=None, sliced=True, wgrad3=None, seed=0,
              launches=None):
    g = _gen(seed * 15485863 + N * 131 + H * 17 + W + Cc + Ko)
    geo = R.Geo(*geo)
    P, Q = R.out_hw(H, W, geo)
    M, T = N * P * Q, geo.R * geo.S
    Creal, Ko_real = Creal or Cc, Ko_real or Ko
    dy = _input(g, M, Ko, dtype, 24 if sliced else 0, 8)
    x = _input(g, N * H * W, Cc, dtype, 8 if sliced else 0, 8)
    old = _randn(g, Ko_real * T * Creal, scale=3.0)
    grad = torch.cat([old, torch.full((T * Creal,), SENT, device=DEV)])     # one sentinel row after the packed gradient
    before = C.wgrad_reduce_launches()
    C.conv2d_wgrad(dy.buf, dy.ld, dy.off, Ko, x.buf, N, H, W, Cc, x.ld, x.off, geo.R, geo.S, geo.stride, geo.pad, P, Q,
                   grad, Creal, Ko_real)
    torch.cuda.synchronize()
    what = f"wgrad {N}x{H}x{W} {Cc}->{Ko} {tuple(geo)} real {Creal}/{Ko_real}"
    if wgrad3 is not None:
        assert C.wgrad3_last() == int(wgrad3), what
    if launches is not None:
        assert C.wgrad_reduce_launches() - before == launches, (what, C.wgrad_reduce_launches() - before)
    assert bool((grad[old.numel():] == SENT).all()), f"{what}: wrote past the packed gradient"
    ref, mag = R.wgrad(dy.v.reshape(N, P, Q, Ko), x.v.reshape(N, H, W, Cc), geo)
    ref, mag = ref[:Ko_real, :, :Creal].reshape(-1), mag[:Ko_real, :, :Creal].reshape(-1)
    # M products summed in any order over the splits and reduce groups (M - 1 additions in all) and the
    # accumulation into the old gradient; fp32 products round
    k = M if dtype == BF16 else 2 * M
    err, tol = (grad[:old.numel()].double() - (old.double() + ref)).abs(), k * U * (old.double().abs() + mag)
    print(f"{what}: {_worst(err, tol)} (k = {k})")
    assert _le(err, tol), f"{what}: {_worst(err, tol)} (k = {k})"


def test_wgrad_gather(C, sw):
    """G: the gather kernel -- 3x3 s2, the 7x7 stem with 3 real channels of 8, 1x1 s2, both row tiles,
    the 64 x 256 tile, fp32, packed [Ko_real][T][Creal] gradients."""
    sw("set_wgrad3", 0)
    run_wgrad(C, 3, 9, 11, 64, 128, G3S2, wgrad3=False, launches=1)            # 128-row tile, 1 split (90 pixels)
    # (at most 297 pixels: one split of max(1, ceil(npix / 512)), one reduce launch)
    run_wgrad(C, 3, 9, 11, 8, 64, G7, Creal=3, wgrad3=False, launches=1)       # 64 x 256 tile (Ko <= 64, TC = 392)
    run_wgrad(C, 3, 9, 11, 8, 64, G7, Creal=3, Ko_real=61, sliced=False, wgrad3=False, launches=1)
    run_wgrad(C, 3, 9, 11, 64, 192, G1S2, Ko_real=190, Creal=59, wgrad3=False, launches=1)
    run_wgrad(C, 3, 9, 11, 64, 64, G3, wgrad3=False, launches=1)               # 64 x 256 tile, TC = 576
    run_wgrad(C, 3, 9, 11, 16, 64, G3, wgrad3=False, Creal=13, launches=1)     # 64 x 128 tile (TC = 144 < 256)
    run_wgrad(C, 3, 9, 11, 32, 64, G3S2, dtype=F32, Creal=29, Ko_real=63, wgrad3=False, launches=1)
    run_wgrad(C, 3, 9, 11, 64, 128, G1, dtype=F32, wgrad3=False, launches=1)


def test_wgrad_direct_1x1(C):
    run_wgrad(C, 3, 9, 11, 64, 128, G1, launches=1)
    run_wgrad(C, 3, 9, 11, 128, 64, G1, Creal=125, Ko_real=60, sliced=False)


@pytest.mark.parametrize("groups", [True, False])
def test_wgrad_gather_splits(C, sw, groups):
    """More than one split, with (a small gradient: two reduce launches) and without reduce groups
    (>= 256k floats: one launch); 3 x 23 x 29 = 2001 pixels, which the 64-aligned pix_per_split does
    not divide."""
    sw("set_wgrad3", 0)
    sw("set_wgrad_blocks", 64)
    if groups:
        run_wgrad(C, 3, 23, 29, 64, 64, G3, wgrad3=False, launches=2)
        run_wgrad(C, 3, 23, 29, 64, 128, G1, launches=2, Creal=61)
    else:
        run_wgrad(C, 3, 23, 29, 256, 128, G3, wgrad3=False, launches=1)


W3 = [(128, 64), (64, 128), (64, 64)]


@pytest.mark.parametrize("Ko,Cc", W3, ids=[f"{k}x{c}" for k, c in W3])
@pytest.mark.parametrize("blocks", [1, 6])
def test_wgrad3(C, sw, Ko, Cc, blocks):
    """The 3x3 spatial-tile kernel in its three tile shapes on 9x11, 8x8 and 17x5 images, with one
    split and with several."""
    sw("set_wgrad3", 1)
    sw("set_wgrad3_blocks", blocks)
    # splits = min(8x8 pixel blocks, target): target `blocks` (twice that for the 4-wave 64 x 64 tile);
    # several splits of a 73,728-float gradient go through reduce groups: two reduce launches
    several = blocks > 1 or (Ko, Cc) == (64, 64)
    for (N, H, W) in ((3, 9, 11), (3, 8, 8), (2, 17, 5)):
        run_wgrad(C, N, H, W, Cc, Ko, G3, wgrad3=True, launches=2 if several else 1)
    run_wgrad(C, 3, 9, 11, Cc, Ko, G3, wgrad3=True, Creal=Cc - 3, Ko_real=Ko - 1, sliced=False,
              launches=2 if several else 1)


# ====================================================================== argument checks on the real binders
def _expect_refusal(fn, prefix):
    with pytest.raises(RuntimeError) as e:
        fn()
    assert prefix in str(e.value), str(e.value)


def test_binders_refuse_what_the_cpu_test_proved(C):
    """Only calls tests/test_conv_args_cpu.py has shown to be refused before a launch reach the real
    binders: its good call with one bad argument, the tensors sized as its element counts say."""
    def buf(numel, dtype=BF16):
        return torch.zeros(max(numel, 1), device=DEV, dtype=dtype)[:max(numel, 0)]

    f32buf = lambda n: buf(n, F32) if n >= 0 else None   # noqa: E731
    opt = lambda n: buf(n) if n >= 0 else None           # noqa: E731
    for what, bad in ARGS.REFUSED_FWD.items():
        a = {**ARGS.FWD, **bad}
        if a["x_numel"] < 0 or a["y_numel"] < 0:
            continue    # (a tensor argument cannot be absent)
        st = None
        if a["stats_rows"] >= 0:
            st = torch.zeros(a["stats_rows"], a["stats_cols"], device=DEV, dtype=F32 if a["stats_f32"] else F64)
        _expect_refusal(lambda: C.conv2d_fwd(
            buf(a["x_numel"]), a["N"], a["H"], a["W"], a["C"], a["ldx"], a["xoff"], buf(a["w_numel"]), a["K"], a["R"],
            a["S"], a["stride"], a["pad"], buf(a["y_numel"]), a["ldy"], a["yoff"], f32buf(a["bias_numel"]),
            opt(a["res_numel"]), a["ldres"], a["resoff"], f32buf(a["scale_numel"]), f32buf(a["shift_numel"]), False,
            st, 0, a["kvalid"], 0), "conv2d_fwd: ")
    for what, bad in ARGS.REFUSED_DGRAD.items():
        a = {**ARGS.DGRAD, **bad}
        if a["dy_numel"] < 0 or a["dx_numel"] < 0:
            continue
        mb = torch.zeros(a["mbits_numel"], device=DEV, dtype=torch.uint8) if a["mbits_numel"] >= 0 else None
        _expect_refusal(lambda: C.conv2d_dgrad_pro(
            buf(a["dy_numel"]), a["N"], a["P"], a["Q"], a["K"], a["lddy"], a["dyoff"], buf(a["wT_numel"]), a["C"],
            a["R"], a["S"], a["stride"], a["pad"], a["H"], a["W"], buf(a["dx_numel"]), a["lddx"], a["dxoff"],
            opt(a["res_numel"]), a["ldres"], a["resoff"], opt(a["mask_numel"]), a["ldmask"], a["maskoff"],
            opt(a["z_numel"]), a["ldz"], a["zoff"], opt(a["z2_numel"]), a["ldz2"], a["z2off"],
            f32buf(a["mscale_numel"]), f32buf(a["mshift_numel"]), mb, a["colsum"], 0, None, None, None, 0, 0,
            f32buf(a["bias_numel"])), "conv2d_dgrad: ")
    for what, bad in ARGS.REFUSED_WGRAD.items():
        a = {**ARGS.WGRAD, **bad}
        if a["dy_numel"] < 0:
            continue
        _expect_refusal(lambda: C.conv2d_wgrad(
            buf(a["dy_numel"]), a["lddy"], a["dyoff"], a["Ko"], buf(a["x_numel"]), a["N"], a["H"], a["W"], a["C"],
            a["ldx"], a["xoff"], a["R"], a["S"], a["stride"], a["pad"], a["P"], a["Q"], buf(a["grad_numel"], F32),
            a["Creal"], a["Ko_real"]), "conv2d_wgrad: ")
