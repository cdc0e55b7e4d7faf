"""Refused arguments of the binders outside the convolutions and BatchNorm (csrc/binding/loss.cpp, optim.cpp,
data.cpp, pool.cpp, ops.cpp): one table of rows = binder, one change to a good argument set, the operand the text
must name and a fragment of the text.  Every row asserts that the RuntimeError carries the binder's name, the
operand's name and the fragment, and that no tensor of the call changed (outputs hold the sentinel 7) once the
device is idle: nothing was launched.  Every binder's good argument set is also called once and must succeed, so
no row passes because the binder refuses everything.  NEW_ROWS / IMAGE_BATCH_ROWS are the calls that the binding
launched before it was split by family (csrc/binding/checks.h).  The integer rules of cls_ce_* are proven without a GPU in
test_cls_ce_cpu.py; the BN family, seg_aug_batch and image_rrc_batch have refusal tables of their own."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, K, HW = 2, 3, 8                     # pixel losses
B, CH, H, W = 2, 3, 4, 4               # image batches
NF, NCHUNK, T = 64, 2, 2               # layer-wise optimisers: 64 floats, two chunks, two tensors


def _native():
    from deeplearning_mpi_amd._ext import native

    return native()


def s7(*shape, dtype=torch.float32):
    return torch.full(shape, 7, dtype=dtype, device=DEV)


def rnd(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).to(DEV)


def i64(values):
    return torch.tensor(values, dtype=torch.int64, device=DEV)


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


# ---- good argument sets, in the binders' argument order ------------------------------------------------------------
def _pix():
    return dict(logits=rnd(N, K, HW), sn=K * HW, sk=HW, sp=1, N=N, K=K, HW=HW,
                labels=i64([0, 1, 2, 1] * (N * HW // 4)), ignore_index=-100, weight=None)


def pixel_ce_fwd():
    return dict(_pix(), lse=s7(N * HW), loss=s7(1), den=s7(1))


def pixel_ce_bwd():
    return dict(_pix(), lse=rnd(N * HW), go=None, den=torch.ones(1, device=DEV), dlogits=s7(N, K, HW))


def seg_counts():
    a = _pix()
    del a["weight"]
    return dict(a, counts=s7(N * K * 3, dtype=torch.int64))


def pixel_ce_dice_fwd():
    return dict(_pix(), ce_weight=1.0, dice_weight=1.0, smooth=1.0, include_background=True, lse=s7(N * HW),
                loss=s7(1), den=s7(1), tab=s7(N * K * 2))


def pixel_ce_dice_bwd():
    return dict(_pix(), lse=rnd(N * HW), go=None, den=torch.ones(1, device=DEV), tab=torch.ones(N * K * 2, device=DEV),
                ce_weight=1.0, dlogits=s7(N, K, HW))


def bce_dice_fwd():
    return dict(logits=rnd(N, HW), target=torch.ones(N, HW, device=DEV), N=N, HW=HW, bce_weight=1.0, dice_weight=1.0,
                smooth=1.0, loss=s7(1), tab=s7(N * 2))


def bce_dice_bwd():
    return dict(logits=rnd(N, HW), target=torch.ones(N, HW, device=DEV), N=N, HW=HW, go=None,
                tab=torch.ones(N * 2, device=DEV), bce_weight=1.0, dlogits=s7(N, HW))


def nhwc_pad_cast():
    return dict(x=rnd(N * HW, K), M=N * HW, K=K, Kp=8, y=s7(N * HW, 8, dtype=torch.bfloat16))


NC, KC = 4, 5                          # classification cross-entropy: rows, classes


def _cls():
    return dict(logits=rnd(NC, KC), ldl=KC, labels=i64([0, 4, 2, 1]), labels_b=None, lam=None, weight=None, N=NC,
                K=KC, ignore_index=-100, eps=0.1)


def cls_ce_fwd():
    return dict(_cls(), lse=s7(NC), rows=s7(3 * NC), loss=s7(1), den=s7(1))


def cls_ce_bwd():
    return dict(_cls(), lse=rnd(NC), rows=torch.ones(3 * NC, device=DEV), den=torch.ones(1, device=DEV), go=None,
                dlogits=s7(NC * KC))


def _lw():                             # chunks [n][4] = {tensor, length, start lo, start hi}
    return dict(chunks=i32([[0, 32, 0, 0], [1, 32, 32, 0]]), flags=i32([0, 0]), extent=NF)


def _tab(fill=0.0):
    return torch.full((_native().lw_tab() + T,), fill, device=DEV)


def seg_sumsq():
    return dict(a=rnd(NF), b=rnd(NF + 1)[1:].contiguous(), **_lw(), partial=s7(2 * NCHUNK))


def seg_finish():
    return dict(partial=torch.ones(2 * NCHUNK, device=DEV), chunk_first=i32([0, 1, 2]), flags=i32([0, 0]),
                tab=_tab(7.0), step=torch.zeros(1, device=DEV), skip=None, mode=0, tc=0.001, wd=1e-4, eps=1e-6,
                b1=0.9, b2=0.999, kind=0, base_lr=0.1, warmup=0.0, total=10.0, min_lr=0.0, power=1.0)


def lars_update():
    return dict(p=rnd(NF), g=rnd(NF), m=s7(NF), **_lw(), tab=_tab(), momentum=0.9, wd=1e-4, nesterov=False)


def lamb_moments():
    return dict(p=rnd(NF), g=rnd(NF), m=s7(NF), v=s7(NF), **_lw(), partial=s7(2 * NCHUNK), tab=_tab(), clip=None,
                b1=0.9, b2=0.999, eps=1e-6, wd=1e-4)


def lamb_update():
    return dict(p=s7(NF), m=rnd(NF), v=torch.ones(NF, device=DEV), **_lw(), tab=_tab(), eps=1e-6, wd=1e-4)


MEAN, STD = [0.5, 0.4, 0.3], [0.2, 0.3, 0.25]


def _images(C=CH):
    data = torch.arange(4 * H * W * C, dtype=torch.int64).remainder(251).to(torch.uint8).view(4, H, W, C).to(DEV)
    return dict(data=data, labels=i64([3, 1, 4, 1]), idx=i64([1, 3]), H=H, W=W, C=C, pad=1, augment=True, seed=5,
                epoch=2, mean=MEAN[:C] + [0.1] * (C - 3), sd=STD[:C] + [0.2] * (C - 3))


def image_batch():
    return dict(_images(), out=s7(B, CH, H, W), out_labels=s7(B, dtype=torch.int64))


def _mix():
    return dict(kind=2, lam=0.75, y0=1, y1=3, x0=0, x1=2)


def image_batch_mix():
    return dict(_images(), **_mix(), out=s7(B, CH, H, W), out_labels=s7(B, dtype=torch.int64),
                labels_b=s7(B, dtype=torch.int64), lam_out=s7(1))


def mix_batch_():
    return dict(x=rnd(B, CH, H, W), labels=i64([3, 1]), **_mix(), labels_b=s7(B, dtype=torch.int64), lam_out=s7(1))


def fill_():
    return dict(t=s7(9), v=1.0)


def add_i64_():
    return dict(t=s7(3, dtype=torch.int64), v=2)


def gather_():
    return dict(dst=s7(8), src=rnd(8), idx=i64([7, -1, 0, 3]), accumulate=False)


def clock_stamp():
    return dict(t=s7(2, 4, dtype=torch.int64))


GOOD = {f.__name__: f for f in (
    pixel_ce_fwd, pixel_ce_bwd, seg_counts, pixel_ce_dice_fwd, pixel_ce_dice_bwd, bce_dice_fwd, bce_dice_bwd,
    nhwc_pad_cast, cls_ce_fwd, cls_ce_bwd, seg_sumsq, seg_finish, lars_update, lamb_moments, lamb_update, image_batch,
    image_batch_mix, mix_batch_, fill_, add_i64_, gather_, clock_stamp)}
PIX = ("pixel_ce_fwd", "pixel_ce_bwd", "seg_counts", "pixel_ce_dice_fwd", "pixel_ce_dice_bwd")
PIX_W = tuple(b for b in PIX if b != "seg_counts")
PIX_BWD = ("pixel_ce_bwd", "pixel_ce_dice_bwd")
LW = ("seg_sumsq", "lars_update", "lamb_moments", "lamb_update")


def strided(t):                        # the same values and shape, every second element of a larger storage
    big = torch.empty(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    big[..., ::2] = t
    return big[..., ::2]


def longer(t):
    return torch.cat([t.reshape(-1), t.reshape(-1)[:1]])


# ---- the rows: (binders, what changes, the change: good arguments -> replaced arguments, operand, fragment) ---------
ROWS = [
    (PIX, "fp64 logits", lambda a: dict(logits=a["logits"].double()), "logits", "fp32"),
    (PIX, "strides past the storage", lambda a: dict(sn=K * HW + 1), "logits", "strides reach outside"),
    (PIX, "K = 1", lambda a: dict(K=1), "logits", "2 <= K <= 256"),
    (PIX, "K = 257", lambda a: dict(K=257), "logits", "2 <= K <= 256"),
    (PIX, "int32 labels", lambda a: dict(labels=a["labels"].int()), "labels", "contiguous int64"),
    (PIX, "strided labels", lambda a: dict(labels=strided(a["labels"])), "labels", "contiguous int64"),
    (PIX, "short labels", lambda a: dict(labels=a["labels"][:-1].contiguous()), "labels", "contiguous int64"),
    (PIX, "host labels", lambda a: dict(labels=a["labels"].cpu()), "labels", "contiguous int64"),
    (PIX_W, "fp64 weight", lambda a: dict(weight=torch.ones(K, dtype=torch.float64, device=DEV)), "weight",
     "contiguous fp32"),
    (PIX_W, "weight [K + 1]", lambda a: dict(weight=torch.ones(K + 1, device=DEV)), "weight", "contiguous fp32"),
    (PIX_W, "long lse", lambda a: dict(lse=longer(a["lse"])), "lse", "contiguous fp32 GPU tensor of 16 elements"),
    (PIX_W, "fp64 lse", lambda a: dict(lse=a["lse"].double()), "lse", "contiguous fp32 GPU tensor of 16 elements"),
    (PIX_W, "den [2]", lambda a: dict(den=s7(2)), "den", "contiguous fp32 GPU tensor of 1 elements"),
    (PIX_W, "fp64 den", lambda a: dict(den=a["den"].double()), "den", "contiguous fp32 GPU tensor of 1 elements"),
    (("pixel_ce_fwd", "pixel_ce_dice_fwd"), "loss [2]", lambda a: dict(loss=s7(2)), "loss",
     "contiguous fp32 GPU tensor of 1 elements"),
    (("pixel_ce_fwd", "pixel_ce_dice_fwd"), "fp64 loss", lambda a: dict(loss=a["loss"].double()), "loss",
     "contiguous fp32 GPU tensor of 1 elements"),
    (("pixel_ce_dice_fwd", "pixel_ce_dice_bwd"), "short tab", lambda a: dict(tab=a["tab"][:-1].contiguous()), "tab",
     "contiguous fp32 GPU tensor of 12 elements"),
    (("pixel_ce_dice_fwd", "pixel_ce_dice_bwd"), "fp64 tab", lambda a: dict(tab=a["tab"].double()), "tab",
     "contiguous fp32 GPU tensor of 12 elements"),
    (("seg_counts",), "short counts", lambda a: dict(counts=a["counts"][:-1].contiguous()), "counts",
     "contiguous int64"),
    (("seg_counts",), "int32 counts", lambda a: dict(counts=a["counts"].int()), "counts", "contiguous int64"),
    (PIX_BWD, "go [2]", lambda a: dict(go=torch.ones(2, device=DEV)), "go", "contiguous fp32 GPU tensor of 1 elements"),
    (PIX_BWD, "dlogits of a smaller storage", lambda a: dict(dlogits=s7(N, K, HW - 1)), "dlogits",
     "strides reach outside"),
    (("pixel_ce_dice_fwd",), "both weights 0", lambda a: dict(ce_weight=0.0, dice_weight=0.0), "weights", "not both 0"),
    (("pixel_ce_dice_fwd",), "smooth = 0", lambda a: dict(smooth=0.0), "smooth", "must be > 0"),
    (("pixel_ce_dice_fwd",), "NaN weight", lambda a: dict(dice_weight=float("nan")), "weights", "must be finite"),
    (("pixel_ce_dice_bwd",), "NaN weight", lambda a: dict(ce_weight=float("nan")), "ce_weight", "must be finite"),

    (("bce_dice_fwd", "bce_dice_bwd"), "short logits", lambda a: dict(logits=a["logits"].reshape(-1)[:-1].contiguous()),
     "logits", "contiguous fp32 GPU tensor of 16 elements"),
    (("bce_dice_fwd", "bce_dice_bwd"), "strided target", lambda a: dict(target=strided(a["target"])), "target",
     "contiguous fp32 GPU tensor of 16 elements"),
    (("bce_dice_fwd", "bce_dice_bwd"), "host tab", lambda a: dict(tab=a["tab"].cpu()), "tab",
     "contiguous fp32 GPU tensor of 4 elements"),
    (("bce_dice_fwd",), "both weights 0", lambda a: dict(bce_weight=0.0, dice_weight=0.0), "weights", "not both 0"),
    (("bce_dice_fwd",), "smooth = 0", lambda a: dict(smooth=0.0), "smooth", "must be > 0"),
    (("bce_dice_bwd",), "strided dlogits", lambda a: dict(dlogits=strided(a["dlogits"])), "dlogits",
     "contiguous fp32 GPU tensor of 16 elements"),
    (("nhwc_pad_cast",), "long x", lambda a: dict(x=longer(a["x"])), "x", "contiguous fp32 GPU tensor of 48 elements"),
    (("nhwc_pad_cast",), "host x", lambda a: dict(x=a["x"].cpu()), "x", "contiguous fp32 GPU tensor of 48 elements"),
    (("nhwc_pad_cast",), "strided y", lambda a: dict(y=strided(a["y"])), "y", "contiguous"),
    (("nhwc_pad_cast",), "short y", lambda a: dict(y=a["y"][:-1].contiguous()), "y", "contiguous"),

    (("cls_ce_fwd", "cls_ce_bwd"), "strided lse", lambda a: dict(lse=strided(a["lse"])), "lse", "contiguous"),
    (("cls_ce_fwd", "cls_ce_bwd"), "host weight", lambda a: dict(weight=torch.ones(KC)), "weight", "GPU tensor"),
    (("cls_ce_fwd", "cls_ce_bwd"), "int32 labels_b",
     lambda a: dict(labels_b=i32([1, 0, 3, 2]), lam=torch.full((1,), 0.5, device=DEV)), "labels", "must be int64"),

    (LW, "chunks [n][3]", lambda a: dict(chunks=a["chunks"][:, :3].contiguous()), "chunks", "must be [n][4]"),
    (LW, "int64 chunks", lambda a: dict(chunks=a["chunks"].long()), "chunks",
     "contiguous int32 GPU tensor of 8 elements"),
    (LW, "empty flags", lambda a: dict(flags=a["flags"][:0]), "flags", "flags [T]"),
    (LW, "extent > n", lambda a: dict(extent=NF + 1), "extent", "the chunk table exceeds the buffers"),
    (("seg_sumsq", "lamb_moments"), "short partial", lambda a: dict(partial=s7(2 * NCHUNK - 1)), "partial",
     "contiguous fp32 GPU tensor of 4 elements"),
    (("lars_update", "lamb_moments", "lamb_update"), "long tab", lambda a: dict(tab=longer(a["tab"])), "tab",
     "contiguous fp32 GPU tensor of"),
    (("lamb_moments",), "clip [1]", lambda a: dict(clip=torch.ones(1, device=DEV)), "clip",
     "contiguous fp32 GPU tensor of 2 elements"),
    (("lamb_moments", "lamb_update"), "eps = 0", lambda a: dict(eps=0.0), "eps", "> 0"),
    (("seg_sumsq",), "b of another length", lambda a: dict(b=rnd(NF - 1)), "b",
     "contiguous fp32 GPU tensor of 64 elements"),
    (("seg_finish",), "empty flags", lambda a: dict(flags=a["flags"][:0]), "flags", "flags [T]"),
    (("seg_finish",), "int64 chunk_first", lambda a: dict(chunk_first=a["chunk_first"].long()), "chunk_first",
     "contiguous int32 GPU tensor of 3 elements"),
    (("seg_finish",), "odd partial", lambda a: dict(partial=torch.ones(2 * NCHUNK - 1, device=DEV)), "partial",
     "must be [2][nchunks]"),
    (("seg_finish",), "long tab", lambda a: dict(tab=longer(a["tab"])), "tab", "contiguous fp32 GPU tensor of"),
    (("seg_finish",), "step [2]", lambda a: dict(step=torch.zeros(2, device=DEV)), "step",
     "contiguous fp32 GPU tensor of 1 elements"),
    (("seg_finish",), "skip [2]", lambda a: dict(skip=torch.zeros(2, device=DEV)), "skip",
     "contiguous fp32 GPU tensor of 1 elements"),
    (("seg_finish",), "mode = 3", lambda a: dict(mode=3), "mode", "mode / kind"),

    (("image_batch_mix", "mix_batch_"), "kind = 3", lambda a: dict(kind=3), "kind", "must be 0, 1 or 2"),
    (("image_batch_mix", "mix_batch_"), "lam = 1.5", lambda a: dict(lam=1.5), "lam", "must lie in [0, 1]"),
    (("image_batch_mix", "mix_batch_"), "box outside the image", lambda a: dict(y1=H + 1), "box",
     "must lie inside the image"),
    (("image_batch_mix", "mix_batch_"), "short labels_b", lambda a: dict(labels_b=s7(B - 1, dtype=torch.int64)),
     "labels_b", "contiguous int64"),
    (("image_batch_mix", "mix_batch_"), "lam_out [2]", lambda a: dict(lam_out=s7(2)), "lam_out",
     "contiguous fp32 GPU tensor of 1 elements"),
    (("image_batch_mix",), "strided out", lambda a: dict(out=strided(a["out"])), "out", "contiguous"),
    (("mix_batch_",), "strided x", lambda a: dict(x=strided(a["x"])), "x", "contiguous fp32"),
    (("image_batch_mix", "image_batch"), "mean of two", lambda a: dict(mean=MEAN[:2]), "mean", "mean/std per channel"),

    (("fill_",), "fp64", lambda a: dict(t=a["t"].double()), "t", "contiguous fp32"),
    (("fill_",), "strided", lambda a: dict(t=strided(a["t"])), "t", "contiguous fp32"),
    (("add_i64_",), "int32", lambda a: dict(t=a["t"].int()), "t", "contiguous int64"),
    (("add_i64_",), "strided", lambda a: dict(t=strided(a["t"])), "t", "contiguous int64"),
    (("clock_stamp",), "int32", lambda a: dict(t=a["t"].int()), "t", "contiguous int64"),
    (("clock_stamp",), "strided", lambda a: dict(t=strided(a["t"])), "t", "contiguous int64"),
    (("clock_stamp",), "[blocks][3]", lambda a: dict(t=s7(2, 3, dtype=torch.int64)), "t", "contiguous int64"),
    (("gather_",), "idx longer than dst", lambda a: dict(idx=i64(list(range(8)) + [0])), "idx", "no longer than dst"),
    (("gather_",), "src of another dtype", lambda a: dict(src=a["src"].double()), "src", "one dtype"),
    (("gather_",), "strided dst", lambda a: dict(dst=strided(a["dst"])), "dst", "contiguous"),
    (("gather_",), "int32 idx", lambda a: dict(idx=a["idx"].int()), "idx", "int64 idx"),
]
# Calls that were launched before the binding was split by family.  image_batch: the preamble it shares with
# image_batch_mix (its `out_labels` stays optional); the utilities: a host tensor.
NEW_ROWS = [
    (("fill_", "add_i64_", "clock_stamp"), "host tensor", lambda a: dict(t=a["t"].cpu()), "t", "GPU tensor"),
]
IMAGE_BATCH_ROWS = [
    ("C = 4", lambda a: dict(_images(4), out=s7(B, 4, H, W)), "channels", "1..3 channels"),
    ("strided out", lambda a: dict(out=strided(a["out"])), "out", "contiguous"),
    ("host idx", lambda a: dict(idx=a["idx"].cpu()), "idx", "contiguous int64"),
    ("int32 labels", lambda a: dict(labels=a["labels"].int()), "labels", "must be int64"),
    ("empty batch", lambda a: dict(idx=a["idx"][:0], out=s7(0, CH, H, W)), "batch", "empty batch"),
]


def _tensors(args):
    return [v for v in args.values() if isinstance(v, torch.Tensor)]


def _refused(binder, what, change, operand, fragment):
    args = GOOD[binder]()
    args.update(change(args))
    before = [t.clone() for t in _tensors(args)]
    with pytest.raises(RuntimeError) as e:
        getattr(_native(), binder)(*args.values())
    text = str(e.value)
    assert text.startswith(binder) and fragment in text, (binder, what, text)
    assert operand in text[len(binder):], (binder, what, text)
    torch.cuda.synchronize()
    for t, b in zip(_tensors(args), before):
        assert torch.equal(t, b), (binder, what)        # nothing was launched


@pytest.mark.parametrize("binder", sorted(GOOD))
def test_good_call_is_accepted(binder):
    args = GOOD[binder]()
    sentinels = [t for t in _tensors(args) if (t == 7).all()]
    getattr(_native(), binder)(*args.values())
    torch.cuda.synchronize()
    assert any(not (t == 7).all() for t in sentinels), binder       # it ran: it wrote something


def _cases(rows):
    return [pytest.param(binder, *row[1:], id=f"{binder}-{row[1]}") for row in rows for binder in row[0]]


def test_every_binder_has_refused_rows():
    assert {b for r in ROWS for b in r[0]} | {"image_batch"} == set(GOOD)


@pytest.mark.parametrize("binder, what, change, operand, fragment", _cases(ROWS))
def test_refused_arguments(binder, what, change, operand, fragment):
    _refused(binder, what, change, operand, fragment)


@pytest.mark.parametrize("binder, what, change, operand, fragment",
                         _cases(NEW_ROWS + [(("image_batch",),) + r for r in IMAGE_BATCH_ROWS]))
def test_newly_refused_arguments(binder, what, change, operand, fragment):
    _refused(binder, what, change, operand, fragment)


def test_image_batch_without_out_labels():
    args = image_batch()
    args["out_labels"] = None
    _native().image_batch(*args.values())
    torch.cuda.synchronize()
    assert not (args["out"] == 7).any()
