"""Timings of the fused CE + Dice loss at the UNet-512 head shape (M = 16 * 512^2 pixels).

Per case -- NHWC logits with K = 2, 3, 21 classes, and the binary (one logit per pixel) case -- the time of
one loss evaluation with its gradient (forward + finish + backward), alternated between
  * ce:        the cross-entropy (BCE) alone, the existing kernels (pixel_ce.hip / loss.hip),
  * ce_dice:   the fused CE + Dice kernels (seg_dice.hip),
  * torch:     the same loss composed from torch ops on the NHWC view (softmax, one_hot, sums, autograd),
with the achieved GB/s over the bytes that must move (logits + labels + lse read or written once forward,
logits + labels + lse + dlogits backward; binary: logits + target, and + dlogits).

Device events over --launches evaluations after a warm-up, --repeats rounds (min / median / max printed).
Usage: python benchmarks/dice_bench.py [--launches 20] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from deeplearning_mpi_amd.ops.backend import NativeBackend  # noqa: E402

DEV = "cuda"


def timed(fn, launches):
    """Mean microseconds per call over `launches` back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def series(fns, launches, repeats):
    """Alternates the candidates, `repeats` rounds: {name: [us per call, ...]}."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(timed(fn, launches))
    return out


def summary(v, nbytes):
    med = statistics.median(v)
    return {"min_us": round(min(v), 1), "median_us": round(med, 1), "max_us": round(max(v), 1),
            "GBps_at_median": round(nbytes / med / 1e3, 1)}


def torch_ce_dice(x, y, K, smooth=1.0):
    p = F.softmax(x, 1)
    oh = F.one_hot(y, K).permute(0, 3, 1, 2).to(x.dtype)
    dice = (2 * (p * oh).sum((2, 3)) + smooth) / (p.sum((2, 3)) + oh.sum((2, 3)) + smooth)
    return F.cross_entropy(x, y) + (1 - dice.mean())


def torch_bce_dice(x, t, smooth=1.0):
    p, tf = torch.sigmoid(x).flatten(1), t.flatten(1)
    dice = (2 * (p * tf).sum(1) + smooth) / (p.sum(1) + tf.sum(1) + smooth)
    return F.binary_cross_entropy_with_logits(x, t) + (1 - dice.mean())


def multiclass(be, K, N, H, W, launches, repeats):
    g = torch.Generator(device=DEV).manual_seed(K)
    M = N * H * W
    x = torch.randn(N, H, W, K, device=DEV, generator=g).permute(0, 3, 1, 2)
    y = torch.randint(K, (N, H, W), device=DEV, generator=g)
    go = torch.ones(1, device=DEV)
    xt = x.detach().clone().requires_grad_(True)   # clone keeps the NHWC strides
    assert xt.stride() == x.stride()

    def ce():
        loss, lse, den = be.pixel_ce_fwd(x, y)
        be.pixel_ce_bwd(x, y, lse, den, go)

    def ce_dice():
        loss, lse, den, tab = be.pixel_ce_dice_fwd(x, y)
        be.pixel_ce_dice_bwd(x, y, lse, den, tab, go)

    def composed():
        xt.grad = None
        torch_ce_dice(xt, y, K).backward()

    nbytes = M * (K * 4 + 8 + 4) + M * (2 * K * 4 + 8 + 4)
    t = series({"ce": ce, "ce_dice": ce_dice, "torch": composed}, launches, repeats)
    res = {k: summary(v, nbytes) for k, v in t.items()}
    return {"case": f"nhwc K={K}", "M": M, "bytes": nbytes, **res,
            "ce_dice_over_ce": round(res["ce_dice"]["median_us"] / res["ce"]["median_us"], 3)}


def binary(be, N, H, W, launches, repeats):
    g = torch.Generator(device=DEV).manual_seed(1)
    M = N * H * W
    x = torch.randn(N, H, W, device=DEV, generator=g)
    t = (torch.rand(N, H, W, device=DEV, generator=g) > 0.5).float()
    go = torch.ones(1, device=DEV)
    xt = x.detach().clone().requires_grad_(True)

    def ce():
        be.bce_fwd(x, t)
        be.bce_bwd(x, t, go)

    def ce_dice():
        loss, tab = be.bce_dice_fwd(x, t)
        be.bce_dice_bwd(x, t, tab, go)

    def composed():
        xt.grad = None
        torch_bce_dice(xt, t).backward()

    nbytes = M * 8 + M * 12
    tt = series({"ce": ce, "ce_dice": ce_dice, "torch": composed}, launches, repeats)
    res = {k: summary(v, nbytes) for k, v in tt.items()}
    return {"case": "binary", "M": M, "bytes": nbytes, **res,
            "ce_dice_over_ce": round(res["ce_dice"]["median_us"] / res["ce"]["median_us"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dice_bench needs the GPU")
    be = NativeBackend(DEV)
    N, H, W = 16, 512, 512
    cases = [multiclass(be, K, N, H, W, a.launches, a.repeats) for K in (2, 3, 21)]
    cases.append(binary(be, N, H, W, a.launches, a.repeats))
    out = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "repeats": a.repeats, "cases": cases}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
