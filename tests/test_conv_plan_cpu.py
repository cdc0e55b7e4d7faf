"""The forward-conv planner (csrc/binding/conv_plan.cpp) without a GPU: the BN-statistics row bound
``conv2d_fwd_mtiles_pro`` against the values recorded from the hand-written mirror ladder it replaced
(fixtures/conv_fwd_rows.json: shape, switch setting, rows), and the invariant whose absence let the two
drift: no plan writes more rows than the bound the caller sized its buffer with."""
import json
import os

import pytest

from deeplearning_mpi_amd._ext import native

C = native()

with open(os.path.join(os.path.dirname(__file__), "fixtures", "conv_fwd_rows.json")) as f:
    FIX = json.load(f)
SWITCHES = FIX["switches"]   # [setter or None, value, value that restores the default]
CASES = FIX["cases"]         # {"shape": [N,H,W,C,K,R,S,stride,pad], "pro", "f32", "bm_req", "rows": one per switch}
AUTOTUNE = [s[0] for s in SWITCHES].index("set_conv_autotune")


@pytest.fixture(params=range(len(SWITCHES)), ids=[f"{s[0]}({s[1]})" if s[0] else "default" for s in SWITCHES])
def switch(request):
    name, val, restore = SWITCHES[request.param]
    if name:
        getattr(C, name)(val)
    yield request.param
    if name:
        getattr(C, name)(restore)


def _bound(c, f32=None):
    return C.conv2d_fwd_mtiles_pro(*c["shape"], c["bm_req"], c["pro"], c["f32"] if f32 is None else f32)


def _rows_m(c, bm):
    N, H, W, _, _, R, S, s, p = c["shape"]
    return -(-(N * ((H + 2 * p - R) // s + 1) * ((W + 2 * p - S) // s + 1)) // bm)


def test_rows_match_the_recorded_ladder(switch):
    """Every recorded row count is reproduced -- except, named here, fp32 with autotuning on, pro 0 and
    free tiles: the old bound sized those for the static tile although the tuner times 64-row fp32
    tiles.  It is now the 64-row count, i.e. the recorded bf16 value of the shape wherever the bf16
    launch is the plain tiled one too (bf16-only kernels -- halo, pipe, streaming -- have other counts)."""
    bf16 = {(tuple(c["shape"]), c["pro"], c["bm_req"]): c["rows"][switch] for c in CASES if not c["f32"]}
    fixed = 0
    for c in CASES:
        want = c["rows"][switch]
        if switch == AUTOTUNE and c["f32"] and c["pro"] == 0 and c["bm_req"] == 0:
            want = _rows_m(c, 64)
            if C.conv2d_fwd_plan(*c["shape"], 0, 0, 0, 0, *_PLAIN(c))["path"] == "igemm":
                assert want == bf16[(tuple(c["shape"]), 0, 0)], c
            fixed += want != c["rows"][switch]
        assert _bound(c) == want, (c, SWITCHES[switch])
    assert (fixed > 0) == (switch == AUTOTUNE)
    if switch == AUTOTUNE:   # the case of the issue: 4 x 128 x 128, 32 -> 64, 1x1
        assert C.conv2d_fwd_mtiles_pro(4, 128, 128, 32, 64, 1, 1, 1, 0, 0, 0, 1) == 1024


def _PLAIN(c):
    """Operand facts "everything aligned, no epilogue": BN statistics + finalize, dense rows."""
    Cc, K = c["shape"][3], c["shape"][4]
    return (False, False, False, True, True, 0, Cc, 0, K, 0)


def _EPILOGUE(c):
    """Operand facts "res + relu, unaligned ldy" (no statistics)."""
    Cc, K = c["shape"][3], c["shape"][4]
    return (True, False, True, False, False, 0, Cc, 0, K + 4, 0)


def test_no_plan_exceeds_the_bound(switch):
    """plan.rows <= conv2d_fwd_mtiles_pro for both operand-fact extremes and, with autotuning on, for
    every tile the tuner may pick."""
    for c in CASES:
        bound = _bound(c)
        head = (*c["shape"], c["pro"], c["f32"], c["bm_req"], 0)
        for facts in (_PLAIN(c), _EPILOGUE(c)):
            if c["pro"] == 3 and facts[0]:
                continue   # a pro-3 consumer has no epilogue of its own (conv2d_fwd_bn_apply)
            plan = C.conv2d_fwd_plan(*head, *facts)
            assert plan["rows"] <= bound, (c, SWITCHES[switch], plan)
        if switch == AUTOTUNE and c["pro"] == 0 and c["bm_req"] == 0:
            plan = C.conv2d_fwd_plan(*head, *_PLAIN(c))
            if plan["path"] != "igemm":
                continue   # the tuner times the plain tiled launch only
            Cc, K = c["shape"][3], c["shape"][4]
            tiles = C.conv_tune_tiles(c["f32"], Cc, K)
            assert (64, 64) in tiles
            for bm, bn in tiles:
                assert not (c["f32"] and (bm > 128 or bn > 128))
                forced = C.conv2d_fwd_plan(*c["shape"], 0, c["f32"], bm, bn if bn < 256 else 0, *_PLAIN(c))
                assert forced["rows"] == _rows_m(c, bm) <= bound, (c, bm, bn)


def test_plan_paths():
    """The ladder picks the kernels the shapes were built for, and falls to the tiled launch when the
    operands rule a persistent kernel out."""
    def path(shape, facts, pro=0, f32=0):
        return C.conv2d_fwd_plan(*shape, pro, f32, 0, 0, *facts)["path"]

    plain = lambda Cc, K: (False, False, False, True, True, 0, Cc, 0, K, 0)    # noqa: E731
    assert path((16, 512, 512, 8, 64, 3, 3, 1, 1), plain(8, 64)) == "c8"
    assert path((256, 115, 115, 16, 64, 4, 4, 1, 0), plain(16, 64)) == "c16"
    assert path((16, 512, 512, 64, 64, 3, 3, 1, 1), plain(64, 64)) == "stream3x3"
    assert path((256, 56, 56, 64, 256, 1, 1, 1, 0), plain(64, 256)) == "stream1x1"
    assert path((256, 56, 56, 64, 256, 1, 1, 1, 0), plain(64, 256), f32=1) == "igemm"
    assert path((256, 56, 56, 64, 256, 1, 1, 1, 0), (True, False, True, False, False, 0, 64, 0, 256, 0)) == "igemm"
    assert path((256, 56, 56, 256, 64, 1, 1, 1, 0), plain(256, 64), pro=3) == "apply1x1"
    assert path((256, 14, 14, 256, 256, 3, 3, 1, 1), plain(256, 256)) == "pipe"
    assert path((16, 128, 128, 256, 256, 3, 3, 1, 1), plain(256, 256)) == "halo"
    assert path((16, 512, 512, 64, 8, 1, 1, 1, 0), (False, False, False, False, False, 1, 64, 0, 1, 0)) == "head"


def test_conv3_pro_ok_needs_room_for_64_channels():
    assert C.conv3_pro_ok(2, 64, 64, 64, 64, 64, 0, 64, 0, 64, 0)
    assert not C.conv3_pro_ok(2, 64, 64, 64, 64, 64, 0, 64, 0, 64, 8)    # applied output: 8 + 64 > 64
    assert not C.conv3_pro_ok(2, 64, 64, 64, 64, 64, 8, 64, 0, 64, 0)    # x: 8 + 64 > 64
    assert C.conv3_pro_ok(2, 64, 64, 64, 64, 128, 64, 64, 0, 128, 64)
