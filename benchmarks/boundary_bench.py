"""Timings of the distance transform and the boundary loss at the UNet-512 head shape (16 x K x 512^2, NHWC view).

Per case -- K = 1 (the sigmoid form), 2, 3, 21:
  * edt:      ops.signed_distance_map alone (edt.hip) on three masks: "blob" (labels in 32 x 32 blocks), "sparse" (a
              1 %-dense random foreground, every other class absent) and "seed" (one foreground pixel in a corner of
              every sample: the column pass's worst case), with the device time of the row and the column kernel;
  * fwd_bwd:  forward + backward of the plain CE / BCE, of ops.ce_boundary_loss / bce_boundary_loss (the transform
              inside) and of the same with a precomputed map (dist=), on the blob mask, alternated;
  * scipy:    scipy.ndimage.distance_transform_edt of the blob mask on the CPU plus the two copies, where scipy is
              installed ("absent" otherwise).
Device events over --launches evaluations after a warm-up, --repeats rounds (min / median / max).
Usage: python benchmarks/boundary_bench.py [--cases 1 2 3 21] [--launches 10] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from benchmarks.ohem_bench import kernel_times, series  # noqa: E402
from deeplearning_mpi_amd import ops  # noqa: E402

DEV = "cuda"
N, S = 16, 512


def masks(K, g):
    """int64 labels [N, S, S] of max(K, 2) classes: blob, sparse, seed."""
    kk = max(K, 2)
    blob = torch.randint(kk, (N, S // 32, S // 32), device=DEV, generator=g)
    blob = blob.repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()
    sparse = (torch.rand(N, S, S, device=DEV, generator=g) < 0.01).long()
    seed = torch.zeros(N, S, S, dtype=torch.int64, device=DEV)
    seed[:, -1, -1] = 1
    return {"blob": blob, "sparse": sparse, "seed": seed}


def scipy_edt(t):
    try:
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        return "absent"
    t0 = time.perf_counter()
    m = t.cpu().numpy() > 0.5
    out = [distance_transform_edt(a) + distance_transform_edt(~a) for a in m]
    torch.as_tensor(out[0]).to(DEV)
    torch.cuda.synchronize()
    return {"planes": len(out), "ms_one_class": round((time.perf_counter() - t0) * 1e3, 1)}


def case(K, launches, repeats):
    g = torch.Generator(device=DEV).manual_seed(K)
    one = torch.ones((), device=DEV)
    ms = masks(K, g)
    as_target = (lambda y: (y > 0).float()) if K == 1 else (lambda y: y)
    sdm = (lambda y: ops.signed_distance_map(as_target(y))) if K == 1 else (lambda y: ops.signed_distance_map(y, K))
    with torch.no_grad():
        edt = series({k: (lambda y=y: sdm(y)) for k, y in ms.items()}, launches, repeats)
        edt_kernels = {k: kernel_times(lambda y=y: sdm(y), calls=3) for k, y in ms.items()}
    y = as_target(ms["blob"])
    if K == 1:
        x = (torch.randn(N, S, S, device=DEV, generator=g) * 3).requires_grad_(True)
        plain = lambda: ops.bce_with_logits(x, y)  # noqa: E731
        dist = ops.signed_distance_map(y)
        fused = lambda: ops.bce_boundary_loss(x, y)  # noqa: E731
        pre = lambda: ops.bce_boundary_loss(x, y, dist=dist)  # noqa: E731
    else:
        x = (torch.randn(N, S, S, K, device=DEV, generator=g) * 3).permute(0, 3, 1, 2).requires_grad_(True)
        plain = lambda: ops.cross_entropy(x, y)  # noqa: E731
        dist = ops.signed_distance_map(y, K)
        fused = lambda: ops.ce_boundary_loss(x, y)  # noqa: E731
        pre = lambda: ops.ce_boundary_loss(x, y, dist=dist)  # noqa: E731

    def fb(f):
        return lambda: torch.autograd.grad(f(), x, one)

    both = series({"plain": fb(plain), "ce+boundary": fb(fused), "ce+boundary_dist": fb(pre)}, launches, repeats)
    kern = kernel_times(fb(fused), calls=3)
    per = N * S * S * K
    return {"K": K, "pixels": N * S * S, "edt": edt, "edt_kernels_us": edt_kernels, "fwd_bwd": both,
            "fwd_bwd_kernels_us": kern,
            "edt_blob_ns_per_pixel_class": round(edt["blob"]["median_us"] * 1e3 / per, 4),
            "scipy_blob": scipy_edt(ms["blob"][:1] > 0) if K == 1 else None}


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
