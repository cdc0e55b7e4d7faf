"""The argument checks of conv2d_fwd / conv2d_dgrad / conv2d_wgrad (csrc/binding/conv_plan.cpp
check_*_args) through their integer-only bindings, without a GPU: one good call per entry point, then
one bad argument at a time for every rule.  tests/test_conv_family_fp64_gpu.py passes the real
binders nothing but calls listed in REFUSED_* here, so a call reaches a GPU only after this file has
shown that it is refused before any launch.

The extent rule (conv_plan.h): (rows - 1) * ld + off + width <= numel and off + width <= ld.
"""
import pytest

from deeplearning_mpi_amd._ext import native

C = native()


def _rows(N, H, W):
    return N * H * W


# the rule each refused call is meant to trip, as a piece of its message: a call must not pass this file
# because some other rule happened to fire.  Keyed by what the case's name begins or ends with.
RULES = [("mask bits", ("mask bits",)), ("absent", ("is required",)), ("short", ("shorter than", "needed")),
         ("not fp32", ("fp32",)), ("columns", ("[rows][2*K]",)), ("no rows", ("[rows][2*K]",)),
         ("alone", ("come together",)), ("empty grid", ("output grid is empty",)),
         ("pad<0", ("pad must not be negative",)), ("stride=3", ("stride <= 2",)),
         ("colsum", ("colsum with a residual",)), ("real", ("Creal / Ko_real",)), ("P ", ("dy grid",)),
         ("Q ", ("dy grid",)), ("H=17", ("dy grid",)), (">ld", ("does not fit its row stride",)),
         ("off<0", ("does not fit its row stride",)), ("=0", ("must be positive",)), ("=-1", ("must be positive",))]


def _names_rule(what, msg):
    """msg holds a piece of the rule the case `what` is about (the first key its name contains)."""
    pieces = next(p for key, p in RULES if key in what)
    return any(p in msg for p in pieces)


# ------------------------------------------------------------------ forward
# 2 x 9 x 11, 16 -> 24 channels, 3x3 / s2 / p1 -> 5 x 6; x a slice [8, 24) of 32, y [8, 32) of 40
FWD = dict(N=2, H=9, W=11, C=16, K=24, R=3, S=3, stride=2, pad=1, kvalid=0,
           x_numel=_rows(2, 9, 11) * 32, ldx=32, xoff=8, w_numel=24 * 9 * 16,
           y_numel=_rows(2, 5, 6) * 40, ldy=40, yoff=8, bias_numel=24,
           res_numel=_rows(2, 5, 6) * 24, ldres=24, resoff=0, scale_numel=24, shift_numel=24,
           stats_rows=4, stats_cols=48, stats_f32=True)
LAST_X = (_rows(2, 9, 11) - 1) * 32 + 8 + 16     # the shortest x the extent rule accepts
LAST_Y = (_rows(2, 5, 6) - 1) * 40 + 8 + 24
REFUSED_FWD = {
    "N=0": dict(N=0), "H=0": dict(H=0), "W=-1": dict(W=-1), "C=0": dict(C=0), "K=0": dict(K=0),
    "R=0": dict(R=0), "S=0": dict(S=0), "stride=0": dict(stride=0), "pad<0": dict(pad=-1),
    "empty grid": dict(H=1, W=1, R=7, S=7, pad=2, w_numel=24 * 49 * 16),
    "xoff+C>ldx": dict(xoff=24), "xoff<0": dict(xoff=-8), "yoff+K>ldy": dict(yoff=24),
    "resoff+K>ldres": dict(resoff=8),
    "x short by one": dict(x_numel=LAST_X - 1), "y short by one": dict(y_numel=LAST_Y - 1),
    "res short by one": dict(res_numel=_rows(2, 5, 6) * 24 - 1),
    "x absent": dict(x_numel=-1), "y absent": dict(y_numel=-1),
    "w short": dict(w_numel=24 * 9 * 16 - 1), "bias short": dict(bias_numel=23),
    "scale short": dict(scale_numel=16), "shift short": dict(shift_numel=8), "scale alone": dict(shift_numel=-1),
    "stats not fp32": dict(stats_f32=False), "stats K columns": dict(stats_cols=24),
    "stats 2K+8 columns": dict(stats_cols=56), "stats no rows": dict(stats_rows=0, stats_cols=0),
}


def test_fwd_good_calls():
    assert C.conv2d_fwd_check(**FWD) == ""
    # the extent rule's edge: buffers that end with the slice of their last row
    assert C.conv2d_fwd_check(**{**FWD, "x_numel": LAST_X, "y_numel": LAST_Y}) == ""
    # every optional operand absent
    plain = {k: v for k, v in FWD.items() if k not in ("bias_numel", "res_numel", "ldres", "resoff", "scale_numel",
                                                        "shift_numel", "stats_rows", "stats_cols", "stats_f32")}
    assert C.conv2d_fwd_check(**plain) == ""
    # kvalid < K stores kvalid channels only: a 3-channel slice of an 11-wide row
    head = {**plain, "kvalid": 3, "ldy": 11, "yoff": 8, "y_numel": (_rows(2, 5, 6) - 1) * 11 + 8 + 3}
    assert C.conv2d_fwd_check(**head) == ""
    assert C.conv2d_fwd_check(**{**head, "y_numel": head["y_numel"] - 1}) != ""
    assert C.conv2d_fwd_check(**{**head, "yoff": 9}) != ""


@pytest.mark.parametrize("what", list(REFUSED_FWD))
def test_fwd_refuses(what):
    msg = C.conv2d_fwd_check(**{**FWD, **REFUSED_FWD[what]})
    assert msg.startswith("conv2d_fwd: ") and _names_rule(what, msg), (what, msg)


# ------------------------------------------------------------------ data gradient
# dy 2 x 8 x 8 x 24 (slice [8, 32) of 40) -> dx 2 x 15 x 15 x 16 (slice [8, 24) of 32), 3x3 / s2 / p1
PIX = _rows(2, 15, 15)
DGRAD = dict(N=2, P=8, Q=8, K=24, C=16, R=3, S=3, stride=2, pad=1, H=15, W=15,
             dy_numel=_rows(2, 8, 8) * 40, lddy=40, dyoff=8, wT_numel=16 * 9 * 24,
             dx_numel=PIX * 32, lddx=32, dxoff=8, res_numel=PIX * 16, ldres=16, resoff=0,
             mask_numel=PIX * 16, ldmask=16, maskoff=0, z_numel=PIX * 24, ldz=24, zoff=8,
             z2_numel=PIX * 16, ldz2=16, z2off=0, mscale_numel=16, mshift_numel=16, mbits_numel=PIX * 2,
             bias_numel=16, colsum=False)
REFUSED_DGRAD = {
    "N=0": dict(N=0), "K=0": dict(K=0), "C=0": dict(C=0), "R=0": dict(R=0), "H=0": dict(H=0),
    "stride=3": dict(stride=3), "stride=0": dict(stride=0),
    "P of H=13": dict(P=7), "Q off by one": dict(Q=9), "H=17 with P=8": dict(H=17),
    "dyoff+K>lddy": dict(dyoff=24), "dxoff+C>lddx": dict(dxoff=24), "resoff+C>ldres": dict(resoff=8),
    "maskoff+C>ldmask": dict(maskoff=8), "zoff+C>ldz": dict(zoff=16), "z2off+C>ldz2": dict(z2off=8),
    "dy short by one": dict(dy_numel=(_rows(2, 8, 8) - 1) * 40 + 8 + 24 - 1),
    "dx short by one": dict(dx_numel=(PIX - 1) * 32 + 8 + 16 - 1),
    "res short": dict(res_numel=PIX * 16 - 1), "mask short": dict(mask_numel=PIX * 16 - 1),
    "z short": dict(z_numel=(PIX - 1) * 24 + 8 + 16 - 1), "z2 short": dict(z2_numel=PIX * 16 - 1),
    "dy absent": dict(dy_numel=-1), "dx absent": dict(dx_numel=-1),
    "wT short": dict(wT_numel=16 * 9 * 24 - 1), "bias short": dict(bias_numel=15),
    "mscale short": dict(mscale_numel=15), "mshift short": dict(mshift_numel=8),
    "mask bits short": dict(mbits_numel=PIX * 2 - 1), "mask bits long": dict(mbits_numel=PIX * 2 + 1),
    # the unmasked column sums are taken before the residual is added: not built together
    "colsum with res": dict(colsum=True, mask_numel=-1, z_numel=-1, z2_numel=-1, mscale_numel=-1, mshift_numel=-1,
                            mbits_numel=-1),
}


def test_dgrad_good_calls():
    assert C.conv2d_dgrad_check(**DGRAD) == ""
    short = {"dy_numel": (_rows(2, 8, 8) - 1) * 40 + 8 + 24, "dx_numel": (PIX - 1) * 32 + 8 + 16,
             "z_numel": (PIX - 1) * 24 + 8 + 16}
    assert C.conv2d_dgrad_check(**{**DGRAD, **short}) == ""
    plain = {k: DGRAD[k] for k in ("N", "P", "Q", "K", "C", "R", "S", "stride", "pad", "H", "W", "dy_numel", "lddy",
                                   "dyoff", "wT_numel", "dx_numel", "lddx", "dxoff")}
    assert C.conv2d_dgrad_check(**plain) == ""
    # column sums without a residual, and with one behind a mask (those are taken after it)
    assert C.conv2d_dgrad_check(**{**plain, "colsum": True}) == ""
    assert C.conv2d_dgrad_check(**{**DGRAD, "colsum": True}) == ""
    # 16 x 15 with the same 8 x 8 dy: another input grid of the same conv
    assert C.conv2d_dgrad_check(**{**plain, "H": 16, "dx_numel": _rows(2, 16, 15) * 32}) == ""
    # 1x1 / s2 on 13 x 14 (7 x 7 outputs)
    assert C.conv2d_dgrad_check(**{**plain, "R": 1, "S": 1, "pad": 0, "H": 13, "W": 14, "P": 7, "Q": 7,
                                   "dy_numel": _rows(2, 7, 7) * 40, "wT_numel": 16 * 24,
                                   "dx_numel": _rows(2, 13, 14) * 32}) == ""


@pytest.mark.parametrize("what", list(REFUSED_DGRAD))
def test_dgrad_refuses(what):
    msg = C.conv2d_dgrad_check(**{**DGRAD, **REFUSED_DGRAD[what]})
    assert msg.startswith("conv2d_dgrad: ") and _names_rule(what, msg), (what, msg)


# ------------------------------------------------------------------ weight gradient
# x 2 x 9 x 11 x 8 (slice [8, 16) of 24), dy 2 x 5 x 6 x 16 (slice [8, 24) of 32), 7x7 / s2 / p3,
# packed gradient [Ko_real = 13][49][Creal = 3]
WGRAD = dict(N=2, H=9, W=11, C=8, Ko=16, R=7, S=7, stride=2, pad=3, P=5, Q=6, Creal=3, Ko_real=13,
             dy_numel=_rows(2, 5, 6) * 32, lddy=32, dyoff=8, x_numel=_rows(2, 9, 11) * 24, ldx=24, xoff=8,
             grad_numel=13 * 49 * 3)
REFUSED_WGRAD = {
    "N=0": dict(N=0), "H=0": dict(H=0), "C=0": dict(C=0), "Ko=0": dict(Ko=0), "S=0": dict(S=0),
    "stride=0": dict(stride=0), "P off by one": dict(P=4), "Q off by one": dict(Q=5),
    "empty grid": dict(H=1, W=1, pad=2, P=0, Q=0),
    "Creal>C real": dict(Creal=9, grad_numel=13 * 49 * 9), "Ko_real>Ko real": dict(Ko_real=17, grad_numel=17 * 49 * 3),
    "Creal<0 real": dict(Creal=-1),
    "dyoff+Ko>lddy": dict(dyoff=24), "xoff+C>ldx": dict(xoff=24),
    "dy short by one": dict(dy_numel=(_rows(2, 5, 6) - 1) * 32 + 8 + 16 - 1),
    "x short by one": dict(x_numel=(_rows(2, 9, 11) - 1) * 24 + 8 + 8 - 1),
    "dy absent": dict(dy_numel=-1), "grad short by one": dict(grad_numel=13 * 49 * 3 - 1),
}


def test_wgrad_good_calls():
    assert C.conv2d_wgrad_check(**WGRAD) == ""
    assert C.conv2d_wgrad_check(**{**WGRAD, "dy_numel": (_rows(2, 5, 6) - 1) * 32 + 8 + 16,
                                   "x_numel": (_rows(2, 9, 11) - 1) * 24 + 8 + 8}) == ""
    assert C.conv2d_wgrad_check(**{**WGRAD, "Creal": 8, "Ko_real": 16, "grad_numel": 16 * 49 * 8}) == ""
    assert C.conv2d_wgrad_check(**{**WGRAD, "Ko_real": 0, "grad_numel": 0}) == ""


@pytest.mark.parametrize("what", list(REFUSED_WGRAD))
def test_wgrad_refuses(what):
    msg = C.conv2d_wgrad_check(**{**WGRAD, **REFUSED_WGRAD[what]})
    assert msg.startswith("conv2d_wgrad: ") and _names_rule(what, msg), (what, msg)
