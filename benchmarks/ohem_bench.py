"""Timings of the OHEM losses at the UNet-512 head shape (M = 16 * 512^2 pixels, NHWC view).

Per case -- K = 1 (binary), 2, 3, 21 -- forward + backward of
  * plain:  the cross-entropy (BCE) alone (pixel_ce.hip / loss.hip),
  * ohem:   ops.ohem_cross_entropy / ohem_bce_with_logits (ohem.hip), with the wave-level aggregation of the histogram
            atomics off (ohem) and on (ohem_agg),
  * torch:  the composition reduction="none" + topk + mask + mean under autograd,
alternated, and the forward alone of plain and ohem.  A profiler run of its own then gives the device time of each
OHEM kernel.  Device events over --launches evaluations after a warm-up, --repeats rounds (min / median / max).
Usage: python benchmarks/ohem_bench.py [--ratio 0.25] [--launches 20] [--repeats 5] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from deeplearning_mpi_amd import ops  # noqa: E402
from deeplearning_mpi_amd._ext import native  # noqa: E402

DEV = "cuda"
N, S = 16, 512


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def series(fns, launches, repeats):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(timed(fn, launches))
    return {k: {"min_us": round(min(v), 1), "median_us": round(statistics.median(v), 1), "max_us": round(max(v), 1)}
            for k, v in out.items()}


def kernel_times(fn, calls=5):
    """Device microseconds per call of every kernel fn launches, by name (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return {e.key.split("(")[0][-60:]: round(e.device_time_total / calls, 1) for e in prof.key_averages()
            if e.device_time_total > 0}


def case(K, ratio, launches, repeats):
    g = torch.Generator(device=DEV).manual_seed(K)
    one = torch.ones((), device=DEV)
    C = native()
    if K == 1:
        x = (torch.randn(N, S, S, device=DEV, generator=g) * 3).requires_grad_(True)
        y = (torch.rand(N, S, S, device=DEV, generator=g) > 0.5).float()
        plain = lambda: ops.bce_with_logits(x, y)  # noqa: E731
        ohem = lambda: ops.ohem_bce_with_logits(x, y, keep_ratio=ratio)  # noqa: E731
        per = lambda: F.binary_cross_entropy_with_logits(x, y, reduction="none").flatten()  # noqa: E731
    else:
        x = (torch.randn(N, S, S, K, device=DEV, generator=g) * 3).permute(0, 3, 1, 2).requires_grad_(True)
        y = torch.randint(K, (N, S, S), device=DEV, generator=g)
        plain = lambda: ops.cross_entropy(x, y)  # noqa: E731
        ohem = lambda: ops.ohem_cross_entropy(x, y, keep_ratio=ratio)  # noqa: E731
        per = lambda: F.cross_entropy(x, y, reduction="none").flatten()  # noqa: E731
    k = math.ceil(ratio * N * S * S)

    def composed():
        l = per()
        cut = torch.topk(l.detach(), k, sorted=True).values[-1]
        m = l.detach() >= cut
        return (l * m).sum() / m.sum()

    def fb(f):
        return lambda: torch.autograd.grad(f(), x, one)

    def agg(f, on):
        def run():
            C.set_ohem_aggregate(on)
            f()
            C.set_ohem_aggregate(0)
        return run

    with torch.no_grad():
        fwd = series({"plain_fwd": plain, "ohem_fwd": ohem, "ohem_agg_fwd": agg(ohem, 1)}, launches, repeats)
    both = series({"plain": fb(plain), "ohem": fb(ohem), "ohem_agg": agg(fb(ohem), 1), "torch": fb(composed)},
                  launches, repeats)
    with torch.no_grad():
        kern = kernel_times(ohem)
    return {"K": K, "pixels": N * S * S, "ratio": ratio, "fwd": fwd, "fwd_bwd": both, "ohem_fwd_kernels_us": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratio", type=float, default=0.25)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"gpu": torch.cuda.get_device_name(0), "cases": [case(K, a.ratio, a.launches, a.repeats) for K in (1, 2, 3, 21)]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
