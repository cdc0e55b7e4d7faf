"""pytorch/resnet/main.py with the recipe flags (label smoothing, mixup, CutMix) on CPU / gloo: one short epoch
to a finite loss, the mixed --benchmark_steps, and the argparser's refusals."""
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--synthetic", "--device", "cpu", "--backend", "gloo", "--workers", "0"]
FLAGS = ["--label_smoothing", "0.1", "--mixup_alpha", "0.2", "--cutmix_alpha", "1.0"]


def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "pytorch/resnet/main.py", *args], cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=timeout)


def _loss(out):
    return float(re.search(r"Epoch: 0, Loss: (\S+)", out).group(1))


def test_one_epoch_with_the_recipe_flags(tmp_path):
    base = [*COMMON, "--num_epochs", "1", "--batch_size", "8", "--synthetic_size", "28", "--model_dir", str(tmp_path)]
    r = _run(base + FLAGS)            # 3 full batches and a ragged one of 4
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    mixed = _loss(r.stdout)
    assert math.isfinite(mixed) and "Epoch 0 completed" in r.stdout and "Accuracy" in r.stdout
    r = _run(base + ["--label_smoothing", "0.1"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    smooth = _loss(r.stdout)
    assert math.isfinite(smooth) and smooth != mixed


def test_benchmark_steps_with_the_recipe_flags():
    r = _run([*COMMON, "--benchmark_steps", "2", "--batch_size", "4", *FLAGS])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "images/sec" in r.stdout


@pytest.mark.parametrize("bad", [["--label_smoothing", "1.0"], ["--label_smoothing", "-0.1"],
                                 ["--label_smoothing", "nan"], ["--mixup_alpha", "-1"], ["--cutmix_alpha", "-0.5"],
                                 ["--mix_prob", "1.5"], ["--mix_switch_prob", "-0.1"]])
def test_invalid_flag_values_are_argparse_errors(bad):
    r = _run([*COMMON, "--num_epochs", "1", *bad], timeout=120)
    assert r.returncode == 2 and "error: " + bad[0] in r.stderr, r.stderr[-2000:]
