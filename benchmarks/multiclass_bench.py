"""Timings of the multi-class segmentation kernels at the UNet-512 head shape (M = 16 * 512^2 pixels).

* head data gradient, C = 64, K = 2 and 4: the streaming kernel (head.hip head_dgrad_bn_kernel) against the
  GEMM path with the reduction padded to 8 -- the two sides of engine._HEAD_DGRAD -- alternated;
* pixel-wise cross-entropy forward / backward, NHWC logits, K = 2 and 21: achieved GB/s over the bytes they
  must move (logits + labels + lse; + dlogits for the backward), beside bn_stats_kernel reading a bf16
  buffer of the same number of bytes, and (K = 21) beside the lane-per-pixel kernels without the LDS tiles.

Device events over --launches launches after a warm-up, --repeats times each (min / median / max printed).
Usage: python benchmarks/multiclass_bench.py [--launches 20] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deeplearning_mpi_amd.models.engine import BwdFuse  # noqa: E402
from deeplearning_mpi_amd.ops.act import Act  # noqa: E402
from deeplearning_mpi_amd.ops.backend import NativeBackend  # noqa: E402

DEV = "cuda"


def timed(fn, launches):
    """Mean microseconds per launch over `launches` back-to-back launches (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def series(fns, launches, repeats):
    """Alternates the candidates, `repeats` rounds: {name: [us per launch, ...]}."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(timed(fn, launches))
    return out


def summary(v):
    return {"min_us": round(min(v), 1), "median_us": round(statistics.median(v), 1), "max_us": round(max(v), 1)}


def head_dgrad(be, K, M, C, launches, repeats):
    g = torch.Generator(device=DEV).manual_seed(K)
    Kp = 8
    dl = torch.zeros(M, Kp, device=DEV, dtype=torch.bfloat16)
    dl[:, :K] = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.zeros(C, Kp, device=DEV, dtype=torch.bfloat16)
    w[:, :K] = (torch.randn(C, K, device=DEV, generator=g) * 0.2).to(torch.bfloat16)
    z = Act(torch.randn(M, C, device=DEV, generator=g).to(torch.bfloat16), 16, 512, M // (16 * 512), C)
    sc, sh = torch.rand(C, device=DEV, generator=g) + 0.5, torch.randn(C, device=DEV, generator=g) * 0.3
    fuse = BwdFuse(None, z, None, sc, sh)
    dla = Act(dl, z.N, z.H, z.W, Kp)
    d1, d2 = Act.empty(z.N, z.H, z.W, C, torch.bfloat16, DEV), Act.empty(z.N, z.H, z.W, C, torch.bfloat16, DEV)
    fns = {"stream": lambda: be.head_dgrad_bn(dla, K, w.view(-1), Kp, d1, fuse),
           "gemm": lambda: be.conv_dgrad(dla, w.view(-1), C, 1, 1, 1, 0, d2, fuse=fuse)}
    t = series(fns, launches, repeats)
    torch.cuda.synchronize()
    same = bool(torch.equal(d1.buf, d2.buf))
    ndiff = int((d1.buf != d2.buf).sum())
    mask_diff = int(((d1.buf == 0) != (d2.buf == 0)).sum())
    both = (d1.buf != 0) & (d2.buf != 0)   # relative difference where neither side is masked
    a, b = d1.buf[both].float(), d2.buf[both].float()
    rel = ((a - b).abs() / b.abs()).max().item() if ndiff and a.numel() else 0.0
    nbytes = M * (Kp * 2 + C * 2 + C * 2)   # dl row + z + dx
    res = {k: summary(v) for k, v in t.items()}
    for k in res:
        res[k]["GBps_at_median"] = round(nbytes / res[k]["median_us"] / 1e3, 1)
    return {"K": K, "M": M, "C": C, "dx_bitwise_equal": same, "dx_elements_differing": ndiff,
            "dx_zero_pattern_differing": mask_diff, "dx_max_rel_diff": rel, **res}


def pixel_ce(be, K, N, H, W, launches, repeats):
    g = torch.Generator(device=DEV).manual_seed(K)
    M = N * H * W
    x = torch.randn(N, H, W, K, device=DEV, generator=g).permute(0, 3, 1, 2)
    y = torch.randint(K, (N, H, W), device=DEV, generator=g)
    go = torch.ones(1, device=DEV)
    loss, lse, den = be.pixel_ce_fwd(x, y)
    b_fwd = M * (K * 4 + 8 + 4)
    b_bwd = M * (2 * K * 4 + 8 + 4)
    rows = b_fwd // (64 * 2)   # bn_stats over a bf16 [rows][64] buffer of the forward's bytes
    sb = Act(torch.randn(rows, 64, device=DEV, generator=g).to(torch.bfloat16), 1, 1, rows, 64)
    def no_tiles(fn):
        def run():
            be.C.set_pixel_tiles(0)
            try:
                fn()
            finally:
                be.C.set_pixel_tiles(1)
        return run

    fns = {"fwd": lambda: be.pixel_ce_fwd(x, y), "bwd": lambda: be.pixel_ce_bwd(x, y, lse, den, go),
           "bn_stats_same_bytes": lambda: be.bn_stats(sb)}
    sizes = [("fwd", b_fwd), ("bwd", b_bwd), ("bn_stats_same_bytes", rows * 128)]
    if K > 4:   # the lane-per-pixel kernels that the LDS tiles replace for class-last logits (A/B)
        fns["fwd_no_tiles"] = no_tiles(fns["fwd"])
        fns["bwd_no_tiles"] = no_tiles(fns["bwd"])
        sizes += [("fwd_no_tiles", b_fwd), ("bwd_no_tiles", b_bwd)]
    t = series(fns, launches, repeats)
    res = {k: summary(v) for k, v in t.items()}
    for k, nb in sizes:
        res[k]["bytes"] = nb
        res[k]["GBps_at_median"] = round(nb / res[k]["median_us"] / 1e3, 1)
    return {"K": K, "M": M, "layout": "nhwc", **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiclass_bench needs the GPU")
    be = NativeBackend(DEV)
    N, H, W = 16, 512, 512
    out = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "repeats": a.repeats,
           "head_dgrad": [head_dgrad(be, K, N * H * W, 64, a.launches, a.repeats) for K in (2, 4)],
           "pixel_ce": [pixel_ce(be, K, N, H, W, a.launches, a.repeats) for K in (2, 21)]}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
