"""Multi-class UNet training on the GPU: the native engine with the pixel-wise cross-entropy against
stock autocast and an fp64 oracle (the scheme of tests/test_models_gpu.py: same slack, floors and skip
rule) for the streaming K = 3 head and the padded-K GEMM head (K = 6), a short training run, hipGraph
replay of a K = 3 step, and the trainer's --num_classes flag."""
import copy
import glob
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from deeplearning_mpi_amd.models import UNet
from deeplearning_mpi_amd.ops import cross_entropy
from deeplearning_mpi_amd.optim import Adam, clip_grad_norm_
from deeplearning_mpi_amd.utils.graphs import CapturedStep

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err(a, ref):
    a, ref = a.double().flatten(), ref.double().flatten()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _compare(make, x, y, loss_e, loss_t, skip=lambda n: False, slack=3.0, floor=2e-2):
    torch.manual_seed(0)
    m1 = make().to(DEV)
    m2 = copy.deepcopy(m1)
    m3 = copy.deepcopy(m1).double()
    for m in (m1, m2, m3):
        m.train()
    o1 = m1(x)
    loss_e(o1, y).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        o2 = m2.forward_torch(x)
    loss_t(o2.float(), y).backward()
    o3 = m3.forward_torch(x.double())
    loss_t(o3, y.double() if y.is_floating_point() else y).backward()
    torch.cuda.synchronize()
    assert _err(o1, o3) <= slack * _err(o2, o3) + 1e-2
    bad = []
    for (n, p1), (_, p2), (_, p3) in zip(m1.named_parameters(), m2.named_parameters(), m3.named_parameters()):
        if skip(n) or p3.grad.abs().max() == 0:
            continue
        e1, e2 = _err(p1.grad, p3.grad), _err(p2.grad, p3.grad)
        if e1 > slack * e2 + floor:
            bad.append((n, round(e1, 4), round(e2, 4)))
    assert not bad, bad
    for (n, b1), (_, b2), (_, b3) in zip(m1.named_buffers(), m2.named_buffers(), m3.named_buffers()):
        if b1.is_floating_point():
            assert _err(b1, b3) <= slack * _err(b2, b3) + 1e-2, n
    m1.eval()
    m3.eval()
    with torch.no_grad():
        assert _err(m1(x), m3.forward_torch(x.double())) < 5e-2


@pytest.mark.parametrize("K,mode", [(3, "conv_transpose"), (3, "bilinear"), (6, "conv_transpose")])
def test_unet_multiclass_engine_vs_autocast(K, mode):
    """K = 3: streaming head forward and the streaming head data gradient; K = 6: the Kp = 8 GEMM head
    both ways."""
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(2, 3, 64, 96, device=DEV, generator=g)
    y = torch.randint(K, (2, 64, 96), device=DEV, generator=g)
    skip = lambda n: n.endswith("bias") and "double_conv.double_conv" in n   # noqa: E731  conv bias before train-BN
    _compare(lambda: UNet(out_classes=K, up_sample_mode=mode), x, y, cross_entropy, F.cross_entropy, skip=skip)


def test_unet_multiclass_training_decreases_loss():
    torch.manual_seed(0)
    m = UNet(out_classes=3, in_channels=1).to(DEV)
    opt = Adam(m.parameters(), lr=1e-3)
    x = torch.randn(2, 1, 64, 64, device=DEV)
    t = (x[:, 0] > 0).long() + (x[:, 0] > 1).long()
    losses = []
    for _ in range(8):
        out = m(x)
        assert out.shape == (2, 3, 64, 64)
        loss = cross_entropy(out, t)
        opt.zero_grad()
        loss.backward()
        clip_grad_norm_(m.parameters(), 1.0, optimizer=opt)
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


def _run_steps(model, batches, graph):
    opt = Adam(model.parameters(), lr=1e-3)
    x, y = batches[0][0].clone(), batches[0][1].clone()

    def step():
        opt.zero_grad()
        loss = cross_entropy(model(x), y)
        loss.backward()
        clip_grad_norm_(model.parameters(), 1.0, optimizer=opt)
        opt.step()
        return loss

    cs = CapturedStep(step, warmup=1, inputs=(x, y), enabled=graph)
    losses = []
    for bx, by in batches:
        cs.set_inputs(bx, by)
        losses.append(cs().clone())
    torch.cuda.synchronize()
    if graph:
        assert cs.graph is not None
    return torch.stack(losses), [p.detach().clone() for p in model.parameters()], \
        [b.detach().clone() for b in model.buffers()]


def test_unet_multiclass_graph_replay_matches_eager():
    """One warm-up step, the capture, two replays: bit-identical to the same four eager steps."""
    g = torch.Generator(device=DEV).manual_seed(4)
    batches = [(torch.randn(2, 3, 64, 64, device=DEV, generator=g),
                torch.randint(3, (2, 64, 64), device=DEV, generator=g)) for _ in range(4)]
    torch.manual_seed(0)
    m1 = UNet(out_classes=3).to(DEV)
    m2 = copy.deepcopy(m1)
    l1, p1, b1 = _run_steps(m1, batches, graph=False)
    l2, p2, b2 = _run_steps(m2, batches, graph=True)
    assert torch.equal(l1, l2), (l1, l2)
    for a, b in zip(p1, p2):
        assert torch.equal(a, b)
    for a, b in zip(b1, b2):
        assert torch.equal(a, b)


def test_trainer_num_classes_3(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "pytorch/unet/train.py", "--synthetic", "--num_classes", "3", "--num_epochs",
                        "1", "--batch_size", "4", "--image_size", "64", "--eval_every", "1", "--workers", "0",
                        "--log_dir", str(tmp_path / "logs"), "--model_dir", str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    (log,) = glob.glob(str(tmp_path / "logs" / "training_log_*.log"))
    lines = [ln for ln in open(log).read().splitlines() if "Dice Score:" in ln]
    assert lines, open(log).read()
    assert 0.0 <= float(lines[0].rsplit(":", 1)[1]) <= 1.0
