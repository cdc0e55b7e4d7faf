"""What the weight EMA (optim.WeightEMA, csrc/kernels/ema.hip) costs.

1. kernels: ``ema_update`` over the ResNet-50 and UNet arenas (flat weights + flat BatchNorm statistics) against the
   ``sgd`` kernel (momentum) on the same arena.  Byte model, fp32 arrays of the arena's size read or written once:
       EMA  w e -> e     3          SGD  w g m -> w m     5          expected ratio 3 / 5 = 0.6
   Device events over --launches back-to-back calls after a warm-up, the two alternated, --repeats rounds
   (min / median / max), GB/s at the median over the byte model.  ``ema_swap`` (4 arrays) is timed beside them.
2. steps: the trainers' --benchmark_steps with and without --ema_decay 0.9999, alternated --rounds times each way in
   processes of their own: ResNet-18 / CIFAR shapes under hipGraph, ResNet-50 224^2 bs 256, UNet 512^2 bs 16.
   A run that does not end with exit status 0 ends the benchmark.

Usage: python benchmarks/ema_bench.py [--what kernels,steps] [--rounds 3] [--out DIR]   (DIR: profiles/weight_ema)
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

import torch  # noqa: E402

DEV = "cuda"
ARRAYS = {"ema_update": 3, "sgd": 5, "ema_swap": 4}
STEP_CASES = {
    "resnet18_cifar_graph": ["pytorch/resnet/main.py", "--synthetic", "--arch", "resnet18", "--batch_size", "128",
                             "--image_size", "32", "--graph", "1", "--benchmark_steps", "400"],
    "resnet50_224_bs256": ["pytorch/resnet/main.py", "--synthetic", "--arch", "resnet50", "--num_classes", "1000",
                           "--batch_size", "256", "--image_size", "224", "--graph", "0", "--benchmark_steps", "60"],
    "unet512_bs16": ["pytorch/unet/train.py", "--synthetic", "--image_size", "512", "--batch_size", "16",
                     "--benchmark_steps", "30"],
}
EMA_FLAGS = ["--ema_decay", "0.9999"]


def timed(fn, launches):
    """Mean microseconds per call over `launches` back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def kernel_case(name, model, launches, repeats):
    from deeplearning_mpi_amd.ops.backend import make_backend
    from deeplearning_mpi_amd.optim import SGD, WeightEMA
    from deeplearning_mpi_amd.utils.arena import ParamArena

    model = model.to(DEV)
    arena = ParamArena(model, DEV, make_backend(DEV))
    g = torch.Generator(device=DEV).manual_seed(1)
    arena.grad.copy_(torch.randn(arena.total, device=DEV, generator=g) * 1e-2)
    for i, p in enumerate(arena.params):   # (the padding between tensors stays zero)
        arena.grad[arena.offsets[i] + p.numel():arena.offsets[i] + (p.numel() + 15) // 16 * 16] = 0
    opt = SGD(list(model.parameters()), lr=1e-7, momentum=0.9, weight_decay=1e-5)   # tiny: the weights stay put
    ema = WeightEMA(model, decay=0.9999, warmup=True, every=1, optimizer=opt)
    for _ in range(3):
        opt.step()
        ema.update()
    assert opt._arena is arena and ema._arena is arena
    be = arena.backend

    def swap():
        be.ema_swap(arena.flat, ema._flat, ema._live_fbuf, ema._fbuf)

    fns = {"ema_update": ema.update, "sgd": opt.step, "ema_swap": swap}
    swap(), swap()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(timed(fn, launches if k != "ema_swap" else launches // 2 * 2))   # an even count: the identity
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ema._flat).all()) and float(ema.state[1]) == 3 + repeats * launches
    res = {}
    for k, v in t.items():
        med = statistics.median(v)
        nbytes = ARRAYS[k] * 4 * (arena.total + (arena.fbuf_total if k != "sgd" else 0))
        res[k] = {"min_us": round(min(v), 1), "median_us": round(med, 1), "max_us": round(max(v), 1),
                  "arrays": ARRAYS[k], "GBps_at_median": round(nbytes / med / 1e3, 1)}
    return {"case": name, "elements": arena.total, "buffer_elements": arena.fbuf_total, **res,
            "ema_over_sgd": round(res["ema_update"]["median_us"] / res["sgd"]["median_us"], 3),
            "byte_model": {"ema_over_sgd": 0.6}}


def kernels(a):
    from deeplearning_mpi_amd.models import UNet, resnet50

    torch.manual_seed(0)
    return [kernel_case("resnet50", resnet50(num_classes=1000), a.launches, a.repeats),
            kernel_case("unet", UNet(out_classes=1), a.launches, a.repeats)]


def one_run(cmd, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, *cmd], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)}: exit status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    m = re.search(r"([0-9.]+) images/sec \(", r.stdout)
    if m is None:
        raise SystemExit(f"{' '.join(cmd)}: no benchmark line\n{r.stdout[-2000:]}")
    ips = float(m.group(1))   # (the printed ms/step has one decimal for the UNet: derive it from the rate)
    return ips, round(1e3 * int(cmd[cmd.index("--batch_size") + 1]) / ips, 4)


def steps(a):
    out = []
    for name in a.cases.split(","):
        cmd = STEP_CASES[name]
        runs = {"off": [], "on": []}
        for _ in range(a.rounds):   # alternated: what else the box is doing drifts under both alike
            runs["off"].append(one_run(cmd, a.run_timeout))
            runs["on"].append(one_run(cmd + EMA_FLAGS, a.run_timeout))
            print(name, "off", runs["off"][-1], "on", runs["on"][-1], flush=True)
        ms = {k: [r[1] for r in v] for k, v in runs.items()}
        med = {k: statistics.median(v) for k, v in ms.items()}
        out.append({"case": name, "command": " ".join(cmd), "ema_flags": " ".join(EMA_FLAGS),
                    "ms_per_step_off": ms["off"], "ms_per_step_on": ms["on"],
                    "images_per_sec_off": [r[0] for r in runs["off"]], "images_per_sec_on": [r[0] for r in runs["on"]],
                    "median_ms_off": med["off"], "median_ms_on": med["on"],
                    "spread_off_percent": round(100 * (max(ms["off"]) - min(ms["off"])) / med["off"], 2),
                    "ema_cost_percent": round(100 * (med["on"] / med["off"] - 1), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernels,steps")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default=",".join(STEP_CASES))
    ap.add_argument("--run_timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_ema"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench needs the GPU")
    os.makedirs(a.out, exist_ok=True)
    for what in a.what.split(","):
        res = {"device": torch.cuda.get_device_name(0)}
        if what == "kernels":
            res.update(launches=a.launches, repeats=a.repeats, cases=kernels(a))
        else:
            res.update(rounds=a.rounds, cases=steps(a))
        txt = json.dumps(res, indent=1)
        print(txt, flush=True)
        with open(os.path.join(a.out, what + ".json"), "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
