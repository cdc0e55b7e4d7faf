"""The classification trainer with label smoothing, mixup and CutMix on the GPU: the replayed hipGraph step
trains like the eager one (the mix runs outside the captured step, into its fixed tensors), and a ResNet-18
step with the new loss launches none but the project's own kernels around it."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _run(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_recipe_graph_matches_eager(tmp_path):
    base = ["pytorch/resnet/main.py", "--synthetic", "--batch_size", "32", "--synthetic_size", "176", "--num_epochs",
            "1", "--workers", "0", "--label_smoothing", "0.1", "--mixup_alpha", "0.2", "--cutmix_alpha", "1.0"]
    out_g = _run(base + ["--model_dir", str(tmp_path / "g"), "--graph", "1"])
    out_e = _run(base + ["--model_dir", str(tmp_path / "e"), "--graph", "0"])
    assert "capture failed" not in out_g
    loss = [re.search(r"Epoch: 0, Loss: (\S+)", o).group(1) for o in (out_g, out_e)]
    assert loss[0] == loss[1] and torch.isfinite(torch.tensor(float(loss[0])))
    wg = torch.load(tmp_path / "g" / "resnet_distributed.pth", weights_only=True)
    we = torch.load(tmp_path / "e" / "resnet_distributed.pth", weights_only=True)
    for k in wg:
        assert torch.equal(wg[k], we[k]), k


def test_resnet_step_launches_no_aten_kernel_on_the_loss_path():
    """engine ResNet-18 + the smoothed, mixed loss: from the average pool's forward to its backward -- the head's
    forward, the loss, the head's weight and data gradients -- only dlmpi:: kernels run."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    from deeplearning_mpi_amd.models import ARCHS
    from deeplearning_mpi_amd.ops import CrossEntropyLoss, backward

    torch.manual_seed(0)
    m = ARCHS["resnet18"](num_classes=10).to(DEV)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    x = torch.randn(8, 3, 32, 32, device=DEV)
    ya, yb = torch.randint(10, (8,), device=DEV), torch.randint(10, (8,), device=DEV)
    lam = torch.full((1,), 0.3, device=DEV)
    backward(crit(m(x), ya, yb, lam))           # warm-up: arena, cached unit seed gradient
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        backward(crit(m(x), ya, yb, lam))
        torch.cuda.synchronize()
    kernels = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
    names = [e.name for e in kernels]
    if not names:
        pytest.fail("the profiler recorded no device kernels")
    first = next(i for i, n in enumerate(names) if "avgpool_fwd_kernel" in n)
    last = next(i for i, n in enumerate(names) if "avgpool_bwd_kernel" in n)
    assert first < last
    between = names[first:last + 1]
    for k in ("cls_ce_fwd_kernel", "cls_ce_finish_kernel", "cls_ce_bwd_kernel"):
        assert sum(k in n for n in between) == 1, (k, between)
    assert not any("softmax_ce" in n for n in names)
    foreign = [n for n in between if "dlmpi::" not in n]
    assert not foreign, foreign
