"""What assembling a RandomResizedCrop batch costs on the GPU.  Run by hand; the results are kept in
profiles/rrc/README.md.

One batch of 256 x 3 x 224 x 224 fp32 from a device-resident set of 1024 uint8 images stored at 256 x 256 and at
144 x 144, through the resampling kernel (csrc/kernels/rrc.hip) with three crop tables:

  identity   the centred 224 x 224 box of every image: one tap of weight 1 per axis (256 store only: a 144 store
             has no 224 box)
  drawn      the table of draw_rrc with the default RrcConfig: scale (0.08, 1), ratio (3/4, 4/3), flip 0.5
  whole      the whole image of every sample: the largest box there is -- at 256 the worst case of the default
             recipe, a 1.14x down-scale with up to 4 x 4 taps; at 144 a 1.56x up-scale
  *_1col     drawn into an output 4 bytes off the 16-byte grid: the kernel's scalar store path

next to three comparisons at the same output bytes:

  image_batch  the crop/flip kernel of the CIFAR pipeline on a 224 x 224 store (one byte read per value written)
  mix_batch    ops.mix_batch_ (mixup) in place on the finished batch: reads and writes it once
  store_floor  the output bytes at the 6.3 TB/s that streaming kernels reach on this part: no kernel that writes
               the batch can be faster

Timings are device events over --launches back-to-back calls after a warm-up, the variants alternated, --repeats
rounds (min / median / max).  Taps per output pixel are counted from the table on the host.
Usage: python benchmarks/rrc_bench.py [--launches N] [--repeats N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deeplearning_mpi_amd.data import (DeviceImageDataset, MixParams, RrcConfig, draw_rrc, mix_batch_,  # noqa: E402
                                       rrc_taps)
from deeplearning_mpi_amd.data.datasets import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402

DEV = "cuda"
N, B, C, S = 1024, 256, 3, 224
STEP_MS = 18.6                   # the ResNet-50 step at batch 256 (README)
STREAM_TBPS = 6.3                # what streaming kernels reach of the HBM's 8 TB/s


def timed(fn, launches):
    """Mean microseconds per call over `launches` back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def alternate(variants, launches, repeats):
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            t[k].append(timed(fn, launches))
    return {k: {"min_us": round(min(v), 2), "median_us": round(statistics.median(v), 2), "max_us": round(max(v), 2)}
            for k, v in t.items()}


def taps_per_pixel(table, idx):
    """Mean taps (source pixels read) per output pixel of the batch, counted from the table."""
    total = 0
    for top, left, h, w, flip in np.asarray(table)[idx].tolist():
        ylo, yhi = rrc_taps(h, S)
        xlo, xhi = rrc_taps(w, S)
        total += int((yhi - ylo).sum()) * int((xhi - xlo).sum())
    return total / (len(idx) * S * S)


class FixedTable(DeviceImageDataset):
    """The resampling dataset with a given table instead of a drawn one."""

    def __init__(self, data, labels, table):
        super().__init__(data, labels, DEV, rrc=RrcConfig(), out_size=S, mean=IMAGENET_MEAN, std=IMAGENET_STD)
        self._table_np = np.ascontiguousarray(table, dtype=np.int32)
        self._table, self._epoch = torch.from_numpy(self._table_np).to(DEV), 0


def bench(store, launches, repeats):
    g = np.random.default_rng(0)
    data = g.integers(0, 256, (N, store, store, C), dtype=np.uint8)
    labels = g.integers(0, 1000, N).astype(np.int64)
    tables = {"drawn": draw_rrc(RrcConfig(), 1, 0, N, store, store),
              "whole": np.tile(np.array([0, 0, store, store, 0], dtype=np.int32), (N, 1))}
    if store >= S:
        o = (store - S) // 2
        tables["identity"] = np.tile(np.array([o, o, S, S, 0], dtype=np.int32), (N, 1))
    sets = {k: FixedTable(data, labels, t) for k, t in tables.items()}
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:B].to(DEV)
    out = (torch.empty(B, C, S, S, device=DEV), torch.empty(B, dtype=torch.int64, device=DEV))
    xb = torch.empty(B * C * S * S + 4, device=DEV)
    off = (xb[1:1 + B * C * S * S].view(B, C, S, S), out[1])
    variants = {k: (lambda ds=ds: ds.batch(idx, 0, out=out)) for k, ds in sets.items()}
    variants["drawn_1col"] = lambda: sets["drawn"].batch(idx, 0, out=off)
    # the comparisons, at the same output bytes
    plain = DeviceImageDataset(g.integers(0, 256, (N, S, S, C), dtype=np.uint8), labels, DEV, augment=True,
                               mean=IMAGENET_MEAN, std=IMAGENET_STD)
    variants["image_batch"] = lambda: plain.batch(idx, 0, out=out)
    mixed = torch.randn(B, C, S, S, device=DEV)
    yb, lam = torch.empty_like(out[1]), torch.empty(1, device=DEV)
    variants["mix_batch"] = lambda: mix_batch_(mixed, out[1], MixParams("mixup", 0.3), yb, lam)
    res = alternate(variants, launches, repeats)
    written = B * C * S * S * 4
    floor_us = written / (STREAM_TBPS * 1e12) * 1e6
    for k, v in res.items():
        v["share_of_resnet50_step"] = round(v["median_us"] / 1e3 / STEP_MS, 4)
        v["over_store_floor"] = round(v["median_us"] / floor_us, 2)
        if k.split("_")[0] in tables:
            v["taps_per_output_pixel"] = round(taps_per_pixel(tables[k.split("_")[0]], idx.cpu().numpy()), 2)
    return {"store": [store, store], "output": [B, C, S, S], "output_bytes": written,
            "store_floor_us": round(floor_us, 2), **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrc_bench needs the GPU")
    out = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "repeats": a.repeats,
           "resnet50_step_ms": STEP_MS, "stream_TBps": STREAM_TBPS,
           "store_256": bench(256, a.launches, a.repeats), "store_144": bench(144, a.launches, a.repeats)}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
