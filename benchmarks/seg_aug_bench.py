"""What assembling an augmented segmentation batch costs on the GPU.  Run by hand; the results are kept in
profiles/seg_aug/README.md.

Batch assembly at 16 x 3 x 512 x 512 from a device-resident set of 64 pairs, float32 masks (the binary trainer)
and int64 masks (class indices), in these variants:

  gathers      DeviceCachedDataset.batch: the two index_select gathers the augmented path replaces (the baseline)
  gathers_out  the same into fixed tensors (what a captured step pays today: gathers + two copies)
  identity     the seg_aug kernel with identity rows (the same pixels as the gathers)
  rot_scale    the seg_aug kernel with a drawn table: flips, scale in [0.8, 1.25], +-30 degrees, +-5 % translation
  *_1col       the last two into outputs one element off the 16-byte grid: the kernel's one-column-per-thread path

Each reports GB/s over a byte model: the output written once, the source read once per tap footprint (the distinct
source pixels a sample's taps touch: all of them for the gathers and the identity, counted from the table for the
drawn transforms).  Timings are device events over --launches back-to-back calls after a warm-up, the variants
alternated, --repeats rounds (min / median / max).
Usage: python benchmarks/seg_aug_bench.py [--launches N] [--repeats N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from deeplearning_mpi_amd.data import DeviceCachedDataset, DeviceSegDataset, SegAugConfig  # noqa: E402

DEV = "cuda"
N, B, C, S = 64, 16, 3, 512
STEP_MS = 16 / 593 * 1e3          # the UNet-512 step at batch 16 (README: 593 img/s)
DRAWN = SegAugConfig(hflip=0.5, vflip=0.5, scale=(0.8, 1.25), rotate=30.0, translate=0.05)


class Pairs:
    """N random image / mask pairs (float 0/1 masks, or int64 class indices for num_classes > 1)."""

    def __init__(self, num_classes):
        g = torch.Generator().manual_seed(0)
        self.images = torch.rand(N, C, S, S, generator=g)
        self.masks = (torch.randint(num_classes, (N, S, S), generator=g) if num_classes > 1
                      else (torch.rand(N, S, S, generator=g) > 0.5).float())

    def __len__(self):
        return N

    def __getitem__(self, i):
        return {"image": self.images[i], "mask": self.masks[i]}


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


def footprint(table, idx, H, W, Ho, Wo):
    """(image pixels, mask pixels) of the source that the batch's taps touch, summed over its samples."""
    t = torch.as_tensor(table).to(torch.int64)[idx.cpu()]
    xs = torch.arange(Wo, dtype=torch.int64).view(1, Wo)
    ys = torch.arange(Ho, dtype=torch.int64).view(Ho, 1)
    img = msk = 0
    for a, b, c, d, e, f in t.tolist():
        X, Y = a * xs + b * ys + c, d * xs + e * ys + f

        def count(ix, iy):
            ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
            return (iy[ok] * W + ix[ok])

        x0, y0 = X >> 16, Y >> 16
        taps = torch.cat([count(x0 + dx, y0 + dy) for dy in (0, 1) for dx in (0, 1)])
        img += taps.unique().numel()
        msk += count((X + 32768) >> 16, (Y + 32768) >> 16).unique().numel()
    return img, msk


def bench(num_classes, launches, repeats):
    src = Pairs(num_classes)
    mb = src.masks.element_size()
    cached = DeviceCachedDataset(src, DEV)
    fill = -100 if num_classes > 1 else None
    ident = DeviceSegDataset(src, DEV, SegAugConfig(), seed=1, mask_fill=fill)
    drawn = DeviceSegDataset(src, DEV, DRAWN, seed=1, mask_fill=fill)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:B].to(DEV)
    out = (torch.empty(B, C, S, S, device=DEV), torch.empty(B, S, S, dtype=src.masks.dtype, device=DEV))
    # the same outputs one element off the 16-byte grid: the kernel's one-column-per-thread path
    xb = torch.empty(B * C * S * S + 4, device=DEV)
    yb = torch.empty(B * S * S + 2, dtype=src.masks.dtype, device=DEV)
    off = (xb[1:1 + B * C * S * S].view(B, C, S, S), yb[1:1 + B * S * S].view(B, S, S))
    ident.table(0), drawn.table(0)   # drawn and copied once per epoch: not part of a step
    res = alternate({"gathers": lambda: cached.batch(idx),
                     "gathers_out": lambda: cached.batch(idx, out=out),
                     "identity": lambda: ident.batch(idx, 0, out=out),
                     "rot_scale": lambda: drawn.batch(idx, 0, out=out),
                     "identity_1col": lambda: ident.batch(idx, 0, out=off),
                     "rot_scale_1col": lambda: drawn.batch(idx, 0, out=off)}, launches, repeats)
    px = B * S * S
    written = px * (C * 4 + mb)
    fi, fm = footprint(drawn.table(0).cpu(), idx, S, S, S, S)
    model = {"gathers": 2 * written, "gathers_out": 4 * written, "identity": 2 * written,
             "rot_scale": written + fi * C * 4 + fm * mb}
    model.update(identity_1col=model["identity"], rot_scale_1col=model["rot_scale"])
    base = res["gathers"]["median_us"]
    for k, v in res.items():
        v["byte_model_bytes"] = model[k]
        v["GBps_at_median"] = round(model[k] / v["median_us"] / 1e3, 1)
        v["over_gathers"] = round(v["median_us"] / base, 3)
        v["share_of_unet512_step"] = round(v["median_us"] / 1e3 / STEP_MS, 4)
    return {"mask_dtype": str(src.masks.dtype), "shape": [B, C, S, S],
            "rot_scale_footprint_share": round(fi / px, 4), **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_aug_bench needs the GPU")
    out = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "repeats": a.repeats,
           "unet512_step_ms": round(STEP_MS, 2),
           "float_masks": bench(1, a.launches, a.repeats), "int64_masks": bench(3, a.launches, a.repeats)}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
