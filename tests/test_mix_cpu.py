"""mixup / CutMix on the host side (data/mix.py) and the CPU path of the device-resident pipeline with a mix."""
import numpy as np
import pytest
import torch

from deeplearning_mpi_amd import ops
from deeplearning_mpi_amd.data import (DeviceBatches, DeviceImageDataset, MixConfig, MixParams, draw_mix,
                                       image_batch_reference, mix_batch_, mix_reference)
from deeplearning_mpi_amd.data.datasets import CIFAR_MEAN, CIFAR_STD

BOTH = MixConfig(mixup_alpha=0.4, cutmix_alpha=1.0)


def test_draw_is_a_function_of_seed_epoch_rank_batch():
    a = draw_mix(BOTH, 3, 2, 1, 17, 32, 32)
    assert a == draw_mix(BOTH, 3, 2, 1, 17, 32, 32)
    draws = {draw_mix(BOTH, 3, 2, r, n, 32, 32) for r in range(4) for n in range(8)}
    assert len(draws) == 32                                 # ranks and batches draw differently
    assert draw_mix(BOTH, 3, 2, 0, 17, 32, 32) != a and draw_mix(BOTH, 4, 2, 1, 17, 32, 32) != a
    assert draw_mix(BOTH, 3, 5, 1, 17, 32, 32) != a


@pytest.mark.parametrize("hw", [(32, 32), (9, 11), (224, 224)])
def test_lam_and_box(hw):
    H, W = hw
    kinds = set()
    for n in range(200):
        p = draw_mix(BOTH, 0, 0, 0, n, H, W)
        kinds.add(p.kind)
        assert 0.0 <= p.lam <= 1.0
        y0, y1, x0, x1 = p.box
        assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
        if p.kind == "cutmix":
            assert p.lam == 1 - (y1 - y0) * (x1 - x0) / (H * W)
        else:
            assert p.box == (0, 0, 0, 0)
    assert kinds == {"mixup", "cutmix"}


def test_single_kinds_prob_and_switch():
    assert {draw_mix(MixConfig(mixup_alpha=1.0), 0, 0, 0, n, 8, 8).kind for n in range(50)} == {"mixup"}
    assert {draw_mix(MixConfig(cutmix_alpha=1.0), 0, 0, 0, n, 8, 8).kind for n in range(50)} == {"cutmix"}
    assert {draw_mix(MixConfig(0.4, 1.0, switch_prob=0.0), 0, 0, 0, n, 8, 8).kind for n in range(50)} == {"mixup"}
    assert {draw_mix(MixConfig(0.4, 1.0, switch_prob=1.0), 0, 0, 0, n, 8, 8).kind for n in range(50)} == {"cutmix"}
    for cfg in (MixConfig(0.4, 1.0, prob=0.0), MixConfig()):
        for n in range(50):
            assert draw_mix(cfg, 0, 0, 0, n, 8, 8) == MixParams("none", 1.0, (0, 0, 0, 0))
    half = [draw_mix(MixConfig(0.4, 1.0, prob=0.5), 0, 0, 0, n, 8, 8).kind for n in range(400)]
    assert 120 < half.count("none") < 280
    assert not MixConfig().enabled and not MixConfig(0.4, prob=0.0).enabled and BOTH.enabled
    for bad in (dict(mixup_alpha=-1.0), dict(cutmix_alpha=float("nan")), dict(prob=1.5), dict(switch_prob=-0.1)):
        with pytest.raises(ValueError):
            MixConfig(**bad)


@pytest.mark.parametrize("B", [1, 2, 7])
def test_mix_reference_semantics(B):
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 3, 9, 11, generator=g)
    y = torch.randint(10, (B,), generator=g)
    lam = 0.3
    out, ya, yb, lt = mix_reference(x, y, MixParams("mixup", lam))
    assert torch.equal(ya, y) and torch.equal(yb, y.flip(0)) and lt.dtype == torch.float32 and float(lt) == np.float32(lam)
    for b in range(B):
        if b == B - 1 - b:
            assert torch.equal(out[b], x[b])                  # its own partner: bit-exactly untouched
        else:
            torch.testing.assert_close(out[b], lam * x[b] + (1 - lam) * x[B - 1 - b], atol=1e-6, rtol=0)
    box = (2, 7, 0, 5)
    out, _, yb, lt = mix_reference(x, y, MixParams("cutmix", 1 - 25 / 99, box))
    inside = torch.zeros(9, 11, dtype=torch.bool)
    inside[2:7, 0:5] = True
    for b in range(B):
        assert torch.equal(out[b], torch.where(inside, x[B - 1 - b], x[b]))
    out, ya, yb, lt = mix_reference(x, y, MixParams())
    assert torch.equal(out, x) and torch.equal(yb, y.flip(0)) and float(lt) == 1.0
    with pytest.raises(ValueError):
        mix_reference(x, y, MixParams("cutmix", 0.5, (0, 10, 0, 5)))


def test_mix_batch_in_place_on_the_cpu():
    x = torch.randn(5, 3, 9, 11)
    y = torch.randint(10, (5,))
    p = MixParams("mixup", 0.7)
    want = mix_reference(x, y, p)
    yb, lam = torch.empty_like(y), torch.empty(1)
    got = ops.mix_batch_(x, y, p, yb, lam)
    assert got[0] is x and got[2] is yb and got[3] is lam and ops.mix_batch_ is mix_batch_
    assert torch.equal(x, want[0]) and torch.equal(yb, want[2]) and torch.equal(lam, want[3])


def _dataset(mix, augment=True, n=40):
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, size=(n, 32, 32, 3), dtype=np.uint8)
    labels = rng.integers(0, 10, size=n)
    return DeviceImageDataset(imgs, labels, "cpu", augment=augment, seed=5, mix=mix)


@pytest.mark.parametrize("augment", [False, True])
def test_cpu_dataset_is_reference_then_mix(augment):
    ds = _dataset(BOTH, augment)
    idx = torch.tensor([3, 9, 1, 30, 22, 17, 8])
    seen = set()
    for no in range(6):
        x, ya, yb, lam = ds.batch(idx, epoch=2, batch_no=no, rank=1)
        p = draw_mix(BOTH, 5, 2, 1, no, 32, 32)
        seen.add(p.kind)
        xr, yr = image_batch_reference(ds.data, ds.labels, idx, 4, augment, 5, 2, CIFAR_MEAN, CIFAR_STD)
        xm, _, ybr, lr = mix_reference(xr, yr, p)
        assert torch.equal(x, xm) and torch.equal(ya, yr) and torch.equal(yb, ybr) and torch.equal(lam, lr)
    assert len(seen) == 2


def test_without_a_mix_the_batch_is_the_pair_of_today():
    ds = _dataset(None)
    idx = torch.tensor([3, 9, 1])
    out = ds.batch(idx, epoch=1)
    assert isinstance(out, tuple) and len(out) == 2
    xr, yr = image_batch_reference(ds.data, ds.labels, idx, 4, True, 5, 1, CIFAR_MEAN, CIFAR_STD)
    assert torch.equal(out[0], xr) and torch.equal(out[1], yr)
    assert all(len(b) == 2 for b in DeviceBatches(ds, 16))


def test_device_batches_number_their_batches_and_fill_four_outputs():
    ds = _dataset(BOTH)
    outs = (torch.empty(16, 3, 32, 32), torch.empty(16, dtype=torch.int64), torch.empty(16, dtype=torch.int64),
            torch.empty(1))
    batches = DeviceBatches(ds, 16, out=outs)
    for no, (x, ya, yb, lam) in enumerate(batches):
        p = draw_mix(BOTH, 5, 0, 0, no, 32, 32)
        assert float(lam) == np.float32(p.lam)
        if x.shape[0] == 16:
            assert x is outs[0] and yb is outs[2] and lam is outs[3]
        assert torch.equal(yb, ya.flip(0))
    assert no == 2
