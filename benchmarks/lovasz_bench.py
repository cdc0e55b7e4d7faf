"""Timings of the Lovasz losses at the UNet-512 head shape (M = 16 * 512^2 pixels, NHWC view).

Per case -- K = 1 (the hinge form), 2, 3, 21 -- forward + backward of
  * plain:   the cross-entropy (BCE) alone (pixel_ce.hip / loss.hip),
  * lovasz:  ops.ce_lovasz_loss / bce_lovasz_loss (lovasz.hip), per_image at the form's default,
  * torch:   the same loss composed from torch ops (softmax, sort, gather, cumsum) under autograd, every class
             counted (classes="present" would need a host read there),
alternated.  A profiler run of its own then gives the device time of each kernel of the lovasz forward + backward,
set against the byte model of profiles/lovasz/README.md.  Device events over --launches evaluations after a warm-up,
--repeats rounds (min / median / max).
Usage: python benchmarks/lovasz_bench.py [--cases 1 2 3 21] [--launches 10] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from benchmarks.ohem_bench import kernel_times, series  # noqa: E402
from deeplearning_mpi_amd import ops  # noqa: E402

DEV = "cuda"
N, S = 16, 512


def jaccard_grad(fgs):
    G = fgs.sum()
    jac = 1 - (G - fgs.cumsum(0)) / (G + (1 - fgs).cumsum(0))
    return torch.cat([jac[:1], jac[1:] - jac[:-1]])


def composed_softmax(x, y, K):
    p = torch.softmax(x, 1)
    segs = []
    for c in range(K):
        fg = (y == c).float().flatten()
        es, perm = torch.sort((fg - p[:, c].flatten()).abs(), descending=True)
        segs.append(torch.dot(es, jaccard_grad(fg[perm])))
    return F.cross_entropy(x, y) + torch.stack(segs).mean()


def composed_hinge(x, t):
    fg = t.flatten(1)
    e = 1 - x.flatten(1) * (2 * fg - 1)
    segs = []
    for n in range(x.shape[0]):
        es, perm = torch.sort(e[n], descending=True)
        segs.append(torch.dot(F.relu(es), jaccard_grad(fg[n][perm])))
    return F.binary_cross_entropy_with_logits(x, t) + torch.stack(segs).mean()


def case(K, launches, repeats):
    g = torch.Generator(device=DEV).manual_seed(K)
    one = torch.ones((), device=DEV)
    if K == 1:
        x = (torch.randn(N, S, S, device=DEV, generator=g) * 3).requires_grad_(True)
        y = (torch.rand(N, S, S, device=DEV, generator=g) > 0.5).float()
        plain = lambda: ops.bce_with_logits(x, y)  # noqa: E731
        lovasz = lambda: ops.bce_lovasz_loss(x, y)  # noqa: E731
        composed = lambda: composed_hinge(x, y)  # noqa: E731
    else:
        x = (torch.randn(N, S, S, K, device=DEV, generator=g) * 3).permute(0, 3, 1, 2).requires_grad_(True)
        y = torch.randint(K, (N, S, S), device=DEV, generator=g)
        plain = lambda: ops.cross_entropy(x, y)  # noqa: E731
        lovasz = lambda: ops.ce_lovasz_loss(x, y)  # noqa: E731
        composed = lambda: composed_softmax(x, y, K)  # noqa: E731

    def fb(f):
        return lambda: torch.autograd.grad(f(), x, one)

    both = series({"plain": fb(plain), "lovasz": fb(lovasz), "torch": fb(composed)}, launches, repeats)
    kern = kernel_times(fb(lovasz), calls=3)
    per = N * S * S * K
    return {"K": K, "pixels": N * S * S, "fwd_bwd": both, "lovasz_kernels_us": kern,
            "lovasz_ns_per_pixel_class": round(both["lovasz"]["median_us"] * 1e3 / per, 3),
            "lovasz_extra_bytes_per_pixel_class_at_4TBs": round(
                (both["lovasz"]["median_us"] - both["plain"]["median_us"]) * 1e-6 * 4e12 / per, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, nargs="+", default=[1, 2, 3, 21])
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"gpu": torch.cuda.get_device_name(0), "cases": [case(K, a.launches, a.repeats) for K in a.cases]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
