"""Timings of ops.surface_distances at the UNet-512 head shape (16 x K x 512^2, NHWC view).

Per case -- K = 1 (the binary form), 3, 21 -- and per input -- "blob" (pred and gt labels drawn per 32 x 32 block,
independently) and "sparse" (a 1 %-dense random foreground in each, every other class absent), the inputs of
benchmarks/boundary_bench.py:
  * op:       ops.surface_distances (edge pass, transform, scan, scatter, select), device events;
  * edt:      the transform inside it on its own: ops' native edt binder on the op's edge-label maps (2 N samples of K
              classes, d2_in only), the maps made beforehand by the torch definition (RefBackend.surface_edges);
  * kernels:  device time per kernel of one op call (torch.profiler, a run of its own);
  * ws_bytes: the op's workspace by the byte model, 12 B per pixel and class + 24 B per pixel (+ tile counts).
Device events over --launches evaluations after a warm-up, --repeats rounds (min / median / max).
Usage: python benchmarks/surface_bench.py [--cases 1 3 21] [--launches 10] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from benchmarks.boundary_bench import masks  # noqa: E402
from benchmarks.ohem_bench import kernel_times, series  # noqa: E402
from deeplearning_mpi_amd import ops  # noqa: E402
from deeplearning_mpi_amd._ext import native  # noqa: E402

DEV = "cuda"
N, S = 16, 512


def logits_of(pred, K, g):
    """Logits whose argmax is ``pred``: class-last storage seen as [N, K, S, S]; the binary form [N, S, S]."""
    if K == 1:
        return torch.where(pred > 0, 1.0, -1.0) * (0.5 + torch.rand(N, S, S, device=DEV, generator=g))
    x = torch.rand(N, S, S, K, device=DEV, generator=g)
    return x.scatter_(3, pred.unsqueeze(3), 2.0).permute(0, 3, 1, 2)


def case(K, launches, repeats):
    g = torch.Generator(device=DEV).manual_seed(K)
    gts, preds = masks(K, g), masks(K, g)
    C, ref = native(), ops.RefBackend(DEV)
    fns, edts, extra = {}, {}, {}
    for name in ("blob", "sparse"):
        y = (gts[name] > 0).float() if K == 1 else gts[name]
        x = logits_of(preds[name], K, g)
        edges = ref.surface_edges(x, y).view(2 * N, S, S).contiguous()
        d2 = torch.empty(2 * N, K, S, S, dtype=torch.int32, device=DEV)
        fns[name] = lambda x=x, y=y: ops.surface_distances(x, y)
        edts[name] = lambda e=edges, d=d2: C.edt(e, K, -1, None, d, None)
        m, c = fns[name]()
        fin = torch.isfinite(m[..., 1])
        extra[name] = {"edge_pixels": int(c.sum()), "finite_rows": int(fin.sum()), "rows": fin.numel(),
                       "mean_hd95": round(m[..., 1][fin].mean().item(), 3) if fin.any() else None}
    op = series(fns, launches, repeats)
    edt = series(edts, launches, repeats)
    kern = {k: kernel_times(f, calls=3) for k, f in fns.items()}
    px = N * S * S
    return {"K": K, "pixels": px, "op": op, "edt_inside": edt, "kernels_us": kern, "inputs": extra,
            "ws_bytes_model": px * (12 * K + 24) + 8 * K * N * (S // 32) ** 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, nargs="+", default=[1, 3, 21])
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
