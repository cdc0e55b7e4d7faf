"""One optimizer step over the ResNet-50 and UNet parameter arenas: SGD (momentum) against LARS,
Adam against LAMB.

Byte model (fp32 arrays of the arena's size read or written once per step):
  SGD   w g m -> w m                 5        LARS  w g | w g m -> w m            7   (1.4 x)
  Adam  w g m v -> w m v             7        LAMB  w g m v -> m v | w m v -> w  10   (1.43 x)
so about 1.4 x the plain optimizer is the floor for either layer-wise one; their middle launch
(seg_finish, one block) and the second kernel boundary come on top.

Device events over --launches steps after a warm-up, the four optimizers alternated, --repeats
rounds (min / median / max printed), GB/s at the median over the byte model.
Usage: python benchmarks/optim_bench.py [--launches 20] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deeplearning_mpi_amd.models import UNet, resnet50  # noqa: E402
from deeplearning_mpi_amd.ops.backend import make_backend  # noqa: E402
from deeplearning_mpi_amd.optim import LAMB, LARS, SGD, Adam  # noqa: E402
from deeplearning_mpi_amd.utils.arena import ParamArena  # noqa: E402

DEV = "cuda"
ARRAYS = {"sgd": 5, "lars": 7, "adam": 7, "lamb": 10}


def timed(fn, launches):
    """Mean microseconds per call over `launches` back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def case(name, model, launches, repeats):
    model = model.to(DEV)
    arena = ParamArena(model, DEV, make_backend(DEV))
    g = torch.Generator(device=DEV).manual_seed(1)
    arena.grad.copy_(torch.randn(arena.total, device=DEV, generator=g) * 1e-2)
    for i, p in enumerate(arena.params):   # (the padding between tensors stays zero)
        arena.grad[arena.offsets[i] + p.numel():arena.offsets[i] + (p.numel() + 15) // 16 * 16] = 0
    w0 = arena.flat.clone()
    ps = list(model.parameters())
    # tiny learning rates: hundreds of timed steps on one gradient leave the weights where they were
    opts = {"sgd": SGD(ps, lr=1e-7, momentum=0.9, weight_decay=1e-5),
            "lars": LARS(ps, lr=1e-4, momentum=0.9, weight_decay=1e-5, trust_coefficient=1e-3),
            "adam": Adam(ps, lr=1e-9),
            "lamb": LAMB(ps, lr=1e-6, weight_decay=0.01)}
    for o in opts.values():
        for _ in range(3):
            o.step()
        assert o._arena is arena
    torch.cuda.synchronize()
    t = {k: [] for k in opts}
    for _ in range(repeats):
        for k, o in opts.items():
            t[k].append(timed(o.step, launches))
    assert torch.isfinite(arena.flat).all() and float((arena.flat - w0).abs().max()) < 1.0
    res = {}
    for k, v in t.items():
        med = statistics.median(v)
        nbytes = ARRAYS[k] * 4 * arena.total
        res[k] = {"min_us": round(min(v), 1), "median_us": round(med, 1), "max_us": round(max(v), 1),
                  "arrays": ARRAYS[k], "GBps_at_median": round(nbytes / med / 1e3, 1)}
    seg = arena.segments()
    return {"case": name, "elements": arena.total, "tensors": len(arena.params), "chunks": seg.nchunks, **res,
            "lars_over_sgd": round(res["lars"]["median_us"] / res["sgd"]["median_us"], 3),
            "lamb_over_adam": round(res["lamb"]["median_us"] / res["adam"]["median_us"], 3),
            "byte_model": {"lars_over_sgd": 1.4, "lamb_over_adam": round(10 / 7, 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs the GPU")
    torch.manual_seed(0)
    cases = [case("resnet50", resnet50(num_classes=1000), a.launches, a.repeats),
             case("unet", UNet(out_classes=1), a.launches, a.repeats)]
    out = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "repeats": a.repeats, "cases": cases}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
