"""Multi-class segmentation on the CPU (reference backend): the pixel-wise cross-entropy and the
engine's K-class head against torch autograd in float64, the integer-mask datasets, and the
trainer's --num_classes flag."""
import copy
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from deeplearning_mpi_amd.data import SegmentationDataset, SyntheticMasks
from deeplearning_mpi_amd.models import UNet, engine
from deeplearning_mpi_amd.ops import (BCEWithLogitsLoss, CrossEntropyLoss, cross_entropy, dice_multiclass, mean_iou,
                                      seg_counts)
from deeplearning_mpi_amd.ops.act import Act
from deeplearning_mpi_amd.ops.backend import RefBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _labels(g, N, K, H, W):
    y = torch.randint(K, (N, H, W), generator=g)
    y[0, :3] = -100          # ignored rows
    y[1, 5, 7] = K + 3       # out of range: ignored as well
    return y


@pytest.mark.parametrize("layout", ["nhwc_view", "nchw"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [2, 5])
def test_pixel_cross_entropy_matches_torch_fp64(K, weighted, layout):
    g = torch.Generator().manual_seed(K)
    N, H, W = 2, 9, 11
    base = torch.randn(N, H, W, K, generator=g, dtype=torch.float64)
    x = base.permute(0, 3, 1, 2) if layout == "nhwc_view" else base.permute(0, 3, 1, 2).contiguous()
    x.requires_grad_(True)
    y = _labels(g, N, K, H, W)
    w = torch.rand(K, generator=g, dtype=torch.float64) + 0.5 if weighted else None
    loss = cross_entropy(x, y, weight=w, ignore_index=-100)
    (gx,) = torch.autograd.grad(loss, x)
    xr = x.detach().clone().requires_grad_(True)
    yr = torch.where((y >= 0) & (y < K), y, torch.full_like(y, -100))
    lr = F.cross_entropy(xr, yr, weight=w, ignore_index=-100)
    (gr,) = torch.autograd.grad(lr, xr)
    assert abs(loss.item() - lr.item()) < 1e-12
    assert (gx - gr).abs().max().item() < 1e-12
    assert gx.stride() == x.stride()
    assert (gx[0, :, :3] == 0).all() and (gx[1, :, 5, 7] == 0).all()


def test_pixel_cross_entropy_other_ignore_index_and_all_ignored():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randint(3, (2, 4, 5), generator=g)
    loss = CrossEntropyLoss(ignore_index=1)(x, y)
    assert abs(loss.item() - F.cross_entropy(x.detach(), y, ignore_index=1).item()) < 1e-12
    # a layout that is neither native one is copied, the gradient still reaches the input
    xs = torch.randn(2, 3, 4, 10, generator=g, dtype=torch.float64, requires_grad=True)
    l2 = cross_entropy(xs[..., ::2], y)
    l2.backward()
    xr = xs.detach().clone().requires_grad_(True)
    F.cross_entropy(xr[..., ::2], y).backward()
    assert (xs.grad - xr.grad).abs().max().item() < 1e-12
    # every pixel ignored: NaN loss, exactly zero gradient (as F.cross_entropy)
    la = cross_entropy(x, torch.full_like(y, -100))
    (ga,) = torch.autograd.grad(la, x)
    assert torch.isnan(la) and (ga == 0).all()
    with pytest.raises(ValueError):
        cross_entropy(x, y.float())


def test_counts_dice_and_iou_reference_backend():
    g = torch.Generator().manual_seed(3)
    N, K, H, W = 2, 4, 6, 7
    x = torch.randn(N, K, H, W, generator=g)
    x[1, 3] = -50.0                       # class 3 never predicted in sample 1 ...
    y = torch.randint(K, (N, H, W), generator=g)
    y[1][y[1] == 3] = 0                   # ... nor present there: scores 1.0
    y[0, 0] = -100
    c = seg_counts(x, y)
    pred = x.argmax(1)
    keep = y != -100
    for n in range(N):
        for k in range(K):
            p, t = (pred[n] == k) & keep[n], (y[n] == k) & keep[n]
            assert c[n, k].tolist() == [int((p & t).sum()), int(p.sum()), int(t.sum())]
    assert c.dtype == torch.int64 and c[1, 3].tolist() == [0, 0, 0]
    cf = c.double()
    want = torch.stack([torch.stack([(2 * cf[n, k, 0] + 1e-8) / (cf[n, k, 1] + cf[n, k, 2] + 1e-8)
                                     if cf[n, k, 1] + cf[n, k, 2] > 0 else torch.tensor(1.0, dtype=torch.float64)
                                     for k in range(1, K)]).mean() for n in range(N)])
    assert torch.allclose(dice_multiclass(x, y).double(), want, atol=1e-6)
    tot = cf.sum(0)
    iou = tot[:, 0] / (tot[:, 1] + tot[:, 2] - tot[:, 0])
    assert abs(mean_iou(x, y).item() - iou.mean().item()) < 1e-6


def _err(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("stream_head", [True, False])
def test_unet_multiclass_train_step_matches_torch(monkeypatch, stream_head):
    """UNet(out_classes=3) in float64, engine + pixel cross-entropy against eager autograd; the head's data
    gradient through head_dgrad_bn (reference form) and through the generic conv_dgrad give the same."""
    monkeypatch.setattr(engine, "_HEAD_DGRAD", stream_head)
    calls = []
    orig = RefBackend.head_dgrad_bn
    monkeypatch.setattr(RefBackend, "head_dgrad_bn", lambda self, *a: calls.append(1) or orig(self, *a))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, 32, 32, generator=g, dtype=torch.float64)
    y = torch.randint(3, (4, 32, 32), generator=g)
    y[0, :2] = -100
    torch.manual_seed(0)
    m1 = UNet(out_classes=3).double()
    m3 = copy.deepcopy(m1)
    m1.train()
    m3.train()
    o1 = m1(x)
    l1 = cross_entropy(o1, y)
    l1.backward()
    o3 = m3.forward_torch(x)
    l3 = F.cross_entropy(o3, y)
    l3.backward()
    assert len(calls) == (1 if stream_head else 0)
    assert _err(o1.detach(), o3.detach()) < 1e-9 and abs(l1.item() - l3.item()) < 1e-9
    for (n, p1), (_, p3) in zip(m1.named_parameters(), m3.named_parameters()):
        if (n.endswith("bias") and "double_conv.double_conv" in n) or p3.grad.abs().max() == 0:
            continue   # conv bias before a training BN: gradient exactly zero
        assert _err(p1.grad, p3.grad) < 1e-9, (n, _err(p1.grad, p3.grad))


@pytest.mark.parametrize("K", [2, 3, 4])
def test_ref_head_dgrad_bn_matches_conv_dgrad(K):
    from deeplearning_mpi_amd.models.engine import BwdFuse

    be = RefBackend("cpu", torch.float64)
    g = torch.Generator().manual_seed(K)
    N, H, W, C, Kp = 1, 5, 7, 16, 8
    dl = Act.zeros(N, H, W, Kp, torch.float64, "cpu")
    dl.nhwc()[..., :K].copy_(torch.randn(N, H, W, K, generator=g, dtype=torch.float64))
    wT = torch.zeros(C, Kp, dtype=torch.float64)
    wT[:, :K] = torch.randn(C, K, generator=g, dtype=torch.float64)
    z = Act(torch.randn(N * H * W, C, generator=g, dtype=torch.float64), N, H, W, C)
    sc, sh = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    fuse = BwdFuse(None, z, None, sc, sh)
    d1, d2 = Act.empty(N, H, W, C, torch.float64, "cpu"), Act.empty(N, H, W, C, torch.float64, "cpu")
    p1 = be.head_dgrad_bn(dl, K, wT.view(-1), Kp, d1, fuse)
    p2 = be.conv_dgrad(dl, wT.view(-1), C, 1, 1, 1, 0, d2, fuse=fuse)
    assert (d1.buf - d2.buf).abs().max().item() < 1e-12 and d1.buf.abs().max() > 0
    assert (p1 - p2).abs().max().item() < 1e-10


def test_integer_mask_datasets(tmp_path):
    rng = np.random.default_rng(0)
    (tmp_path / "images").mkdir()
    (tmp_path / "masks").mkdir()
    masks = []
    for i in range(3):
        np.save(tmp_path / "images" / f"s{i}.npy", rng.integers(0, 255, (8, 10, 3), dtype=np.uint8))
        m = rng.choice(np.array([0, 90, 255], dtype=np.uint8), size=(8, 10))
        masks.append(m)
        np.save(tmp_path / "masks" / f"s{i}.npy", m)
    multi = SegmentationDataset(tmp_path / "images", tmp_path / "masks", multiclass=True)
    plain = SegmentationDataset(tmp_path / "images", tmp_path / "masks")
    assert multi.mask_values == [0, 90, 255]
    for i in range(3):
        t = multi[i]["mask"]
        assert t.dtype == torch.int64 and t.shape == (8, 10)
        assert torch.equal(t, torch.from_numpy(multi.mask_indices(masks[i])))
        assert set(t.unique().tolist()) <= {0, 1, 2} and t.max() == 2
        b = plain[i]["mask"]   # the default stays the binarised float mask
        assert b.dtype == torch.float32 and torch.equal(b, (t > 0).float())
        assert torch.equal(plain[i]["image"], multi[i]["image"])
    s4 = SyntheticMasks(4, (3, 16, 16), seed=7, num_classes=4)[1]["mask"]
    assert s4.dtype == torch.int64 and s4.shape == (16, 16) and 0 <= int(s4.min()) and int(s4.max()) == 3
    # default arguments: today's samples exactly (same generator draws)
    a = SyntheticMasks(4, (3, 16, 16), seed=7)[1]
    gen = torch.Generator().manual_seed(7 * 1000003 + 1)
    img = torch.rand((3, 16, 16), generator=gen)
    msk = (torch.rand((16, 16), generator=gen) > 0.5).float()
    assert torch.equal(a["image"], img) and torch.equal(a["mask"], msk) and a["mask"].dtype == torch.float32


def test_device_cached_dataset_keeps_int64_masks():
    from deeplearning_mpi_amd.data import DeviceBatches, DeviceCachedDataset

    ds = DeviceCachedDataset(SyntheticMasks(5, (3, 16, 16), num_classes=3), "cpu")
    out = (torch.zeros(2, 3, 16, 16), torch.zeros(2, 16, 16, dtype=torch.int64))
    batches = list(DeviceBatches(ds, 2, out=out))
    assert batches[0]["mask"].dtype == torch.int64 and batches[0]["mask"] is out[1]
    assert batches[-1]["mask"].dtype == torch.int64 and batches[-1]["mask"].shape == (1, 16, 16)


def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_trainer_num_classes_3_on_cpu(tmp_path):
    logs = tmp_path / "logs"
    r = _run([sys.executable, "pytorch/unet/train.py", "--device", "cpu", "--backend", "gloo", "--synthetic",
              "--num_classes", "3", "--image_size", "32", "--num_epochs", "1", "--workers", "0", "--batch_size", "2",
              "--synthetic_size", "6", "--eval_every", "1", "--log_dir", str(logs), "--model_dir", str(tmp_path)])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    (log,) = glob.glob(str(logs / "training_log_*.log"))
    line = [ln for ln in open(log).read().splitlines() if "Dice Score:" in ln][0]
    assert 0.0 <= float(line.rsplit(":", 1)[1]) <= 1.0
    sd = torch.load(tmp_path / "model.pth", weights_only=True)
    assert sd["module.conv_last.weight"].shape == (3, 64, 1, 1)


def test_trainer_rejects_more_mask_values_than_classes(tmp_path):
    rng = np.random.default_rng(0)
    (tmp_path / "images").mkdir()
    (tmp_path / "masks").mkdir()
    for i in range(5):
        np.save(tmp_path / "images" / f"s{i}.npy", rng.integers(0, 255, (16, 16, 3), dtype=np.uint8))
        np.save(tmp_path / "masks" / f"s{i}.npy", rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=(16, 16)))
    r = _run([sys.executable, "pytorch/unet/train.py", "--device", "cpu", "--backend", "gloo", "--num_classes", "3",
              "--data_dir", str(tmp_path), "--scale", "1.0", "--num_epochs", "1", "--workers", "0",
              "--log_dir", str(tmp_path / "logs"), "--model_dir", str(tmp_path)])
    assert r.returncode != 0
    assert "4 distinct values" in r.stderr and "--num_classes 3" in r.stderr


def test_num_classes_1_builds_todays_model_and_loss(monkeypatch, tmp_path):
    """The default keeps UNet(out_classes=1) + BCEWithLogitsLoss and float masks; K > 1 switches all three."""
    from deeplearning_mpi_amd.apps import segmentation as seg

    assert seg.build_argparser().parse_args([]).num_classes == 1
    seen = {}

    class Stop(Exception):
        pass

    def fake_use_graph(args, device, **kw):
        raise Stop

    real_unet, real_bce, real_ce = seg.UNet, seg.BCEWithLogitsLoss, seg.CrossEntropyLoss
    monkeypatch.setattr(seg, "UNet", lambda **kw: seen.setdefault("model", real_unet(**kw)))
    monkeypatch.setattr(seg, "BCEWithLogitsLoss", lambda **kw: seen.setdefault("crit", real_bce(**kw)))
    monkeypatch.setattr(seg, "CrossEntropyLoss", lambda **kw: seen.setdefault("crit", real_ce(**kw)))
    monkeypatch.setattr(seg, "use_graph", fake_use_graph)
    for k, crit in ((1, BCEWithLogitsLoss), (3, CrossEntropyLoss)):
        seen.clear()
        args = seg.build_argparser().parse_args(["--device", "cpu", "--backend", "gloo", "--synthetic", "--image_size",
                                                 "32", "--synthetic_size", "4", "--num_classes", str(k), "--log_dir",
                                                 str(tmp_path)])
        with pytest.raises(Stop):
            seg.run(args)
        seg.parallel.destroy_distributed()
        assert type(seen["model"]) is UNet and seen["model"].out_classes == k
        assert type(seen["crit"]) is crit
