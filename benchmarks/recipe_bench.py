"""What the classification recipe (label smoothing, mixup, CutMix) costs on the GPU.  Run by hand; the results
are kept in profiles/cls_recipe/README.md.

  loss    forward + backward of the classification loss: the plain kernels (every default) against the
          cls_ce kernels (label smoothing 0.1 + a mixed target), at (N, K) = (128, 10) and (256, 1000)
  batch   the device-resident CIFAR batch kernel at batch size 128, without and with the fused mix
  mix     ops.mix_batch_ on 256 x 3 x 224 x 224: GB/s over its byte model (the batch read and written once)
  steps   pytorch/resnet/main.py --benchmark_steps for resnet18 / CIFAR and resnet50 / 224, without and with the
          recipe flags, each in a child process; --parent DIR adds the same default run from another checkout
          (the parent commit, built) as the yardstick for the defaults

Kernel timings are device events over --launches back-to-back calls after a warm-up, the variants alternated,
--repeats rounds (min / median / max).
Usage: python benchmarks/recipe_bench.py [--only loss,batch,mix,steps] [--parent DIR] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deeplearning_mpi_amd import ops  # noqa: E402
from deeplearning_mpi_amd.data import DeviceImageDataset, MixConfig, MixParams  # noqa: E402

DEV = "cuda"
FLAGS = ["--label_smoothing", "0.1", "--mixup_alpha", "0.2", "--cutmix_alpha", "1.0"]


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


def bench_loss(launches, repeats):
    out = []
    for N, K in ((128, 10), (256, 1000)):
        g = torch.Generator(device=DEV).manual_seed(N)
        x = torch.randn(N, K, device=DEV, generator=g).requires_grad_(True)
        a = torch.randint(K, (N,), device=DEV, generator=g)
        b = a.flip(0).contiguous()
        lam = torch.full((1,), 0.3, device=DEV)

        def plain():
            ops.backward(ops.cross_entropy(x, a))
            x.grad = None

        def recipe():
            ops.backward(ops.cross_entropy(x, a, label_smoothing=0.1, labels_b=b, lam=lam))
            x.grad = None

        out.append({"N": N, "K": K, **alternate({"plain_fwd_bwd": plain, "recipe_fwd_bwd": recipe}, launches, repeats)})
    return out


def bench_batch(launches, repeats):
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, size=(50000, 32, 32, 3), dtype=np.uint8)
    labels = rng.integers(0, 10, size=50000)
    idx = torch.as_tensor(rng.permutation(50000)[:128]).to(DEV)
    plain = DeviceImageDataset(imgs, labels, DEV, augment=True, seed=1)
    mixed = DeviceImageDataset(imgs, labels, DEV, augment=True, seed=1, mix=MixConfig(0.2, 1.0))
    o2 = plain.batch(idx)
    o4 = mixed.batch(idx)
    res = alternate({"batch": lambda: plain.batch(idx, 1, out=o2),
                     "batch_mixed": lambda: mixed.batch(idx, 1, out=o4, batch_no=3)}, launches, repeats)
    return {"B": 128, "note": "batch_mixed includes the host-side draw of the mix", **res}


def bench_mix(launches, repeats):
    x = torch.randn(256, 3, 224, 224, device=DEV)
    y = torch.randint(1000, (256,), device=DEV)
    yb, lam = torch.empty_like(y), torch.empty(1, device=DEV)
    cut = MixParams("cutmix", 1 - 112 * 112 / (224 * 224), (50, 162, 60, 172))
    res = alternate({"mixup": lambda: ops.mix_batch_(x, y, MixParams("mixup", 0.3), yb, lam),
                     "cutmix": lambda: ops.mix_batch_(x, y, cut, yb, lam)}, launches, repeats)
    nbytes = 2 * x.numel() * 4   # the byte model: every element read once and written once
    for v in res.values():
        v["GBps_at_median"] = round(nbytes / v["median_us"] / 1e3, 1)
    return {"shape": list(x.shape), "byte_model_bytes": nbytes,
            "note": "CutMix needs only the box (a quarter of the image here); the kernel still sweeps the batch", **res}


def bench_steps(parent, steps, repeats):
    cases = {"resnet18_cifar_bs128": ["--arch", "resnet18", "--batch_size", "128", "--image_size", "32"],
             "resnet50_224_bs256": ["--arch", "resnet50", "--batch_size", "256", "--image_size", "224",
                                    "--num_classes", "1000"]}
    out = {}
    for name, args in cases.items():
        variants = {"defaults": (ROOT, []), "recipe": (ROOT, FLAGS)}
        if parent:
            variants = {"parent_defaults": (os.path.abspath(parent), []), **variants}
        ips = {k: [] for k in variants}
        for _ in range(repeats):
            for k, (root, extra) in variants.items():
                env = dict(os.environ, PYTHONPATH=root)
                r = subprocess.run([sys.executable, "pytorch/resnet/main.py", "--synthetic", "--benchmark_steps",
                                    str(steps), *args, *extra], cwd=root, env=env, capture_output=True, text=True,
                                   timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"{name} {k} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
                ips[k].append(float(re.search(r"steps: ([0-9.]+) images/sec", r.stdout).group(1)))
                print(name, k, ips[k][-1], flush=True)
        out[name] = {k: {"images_per_sec": v, "median": statistics.median(v)} for k, v in ips.items()}
        med = {k: v["median"] for k, v in out[name].items()}
        out[name]["recipe_over_defaults"] = round(med["recipe"] / med["defaults"], 4)
        if parent:
            out[name]["defaults_over_parent"] = round(med["defaults"] / med["parent_defaults"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="loss,batch,mix,steps")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=60, help="--benchmark_steps of each step run")
    ap.add_argument("--step_repeats", type=int, default=3)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit (steps: the yardstick)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recipe_bench needs the GPU")
    only = a.only.split(",")
    out = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "repeats": a.repeats}
    if "loss" in only:
        out["loss"] = bench_loss(a.launches, a.repeats)
    if "batch" in only:
        out["batch"] = bench_batch(a.launches, a.repeats)
    if "mix" in only:
        out["mix"] = bench_mix(max(10, a.launches // 10), a.repeats)
    if "steps" in only:
        out["steps"] = bench_steps(a.parent, a.steps, a.step_repeats)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
