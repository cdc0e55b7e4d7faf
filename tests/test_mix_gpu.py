"""mixup / CutMix on the device (csrc/kernels/data.hip) against the torch reference: the batch kernel of the
device-resident pipeline with the mix fused in, and the in-place kernel for any fp32 NCHW batch.

mixup blends normalised values (|v| < 2.8, one fp32 step 2.4e-7) with one fused multiply-add where torch rounds
twice: atol 1e-6, the bound of tests/test_device_data.py.  CutMix only moves values: bit-exact."""
import numpy as np
import pytest
import torch

from deeplearning_mpi_amd.data import (DeviceImageDataset, MixConfig, MixParams, draw_mix, image_batch_reference,
                                       mix_batch_, mix_reference)
from deeplearning_mpi_amd.data.datasets import CIFAR_MEAN, CIFAR_STD

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = W = 32
# mixup, CutMix boxes that touch each edge, one inside, an empty box (lam = 1), the full image (lam = 0), no mix
CASES = [MixParams("mixup", 0.3), MixParams("mixup", 1.0), MixParams("mixup", 0.0),
         MixParams("cutmix", 1 - 5 * 9 / 1024, (0, 5, 7, 16)), MixParams("cutmix", 1 - 5 * 9 / 1024, (27, 32, 7, 16)),
         MixParams("cutmix", 1 - 5 * 9 / 1024, (7, 16, 0, 5)), MixParams("cutmix", 1 - 5 * 9 / 1024, (7, 16, 27, 32)),
         MixParams("cutmix", 1 - 6 * 6 / 1024, (10, 16, 3, 9)), MixParams("cutmix", 1.0, (4, 4, 9, 9)),
         MixParams("cutmix", 0.0, (0, 32, 0, 32)), MixParams()]
RNG = np.random.default_rng(0)
IMGS = RNG.integers(0, 256, size=(300, H, W, 3), dtype=np.uint8)
LABELS = RNG.integers(0, 10, size=300)


def _check(got, want, kind):
    x, ya, yb, lam = (t.cpu() for t in got)
    if kind == "mixup":
        torch.testing.assert_close(x, want[0], atol=1e-6, rtol=0)
    else:
        assert torch.equal(x, want[0])
    assert torch.equal(ya, want[1]) and torch.equal(yb, want[2]) and torch.equal(lam, want[3])


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("B", [1, 7, 128])
def test_fused_batch_kernel(B, augment, monkeypatch):
    import deeplearning_mpi_amd.data.device as device

    ds = DeviceImageDataset(IMGS, LABELS, DEV, augment=augment, seed=5, mix=MixConfig(0.4, 1.0))
    idx = torch.as_tensor(np.random.default_rng(B).permutation(300)[:B])
    xr, yr = image_batch_reference(torch.as_tensor(IMGS), torch.as_tensor(LABELS), idx, 4, augment, 5, 2, CIFAR_MEAN,
                                   CIFAR_STD)
    for p in CASES:
        monkeypatch.setattr(device, "draw_mix", lambda *a, p=p: p)
        out = (torch.full(xr.shape, 7.0, device=DEV), torch.full_like(yr, 7).to(DEV), torch.full_like(yr, 7).to(DEV),
               torch.full((1,), 7.0, device=DEV))                                        # the kernel writes all four
        got = ds.batch(idx.to(DEV), epoch=2, out=out)
        assert got[0] is out[0] and got[3] is out[3]
        _check(got, mix_reference(xr, yr, p), p.kind)
        if B % 2:    # the middle sample is its own partner: bit-exactly the unmixed one
            assert torch.equal(got[0][B // 2].cpu(), xr[B // 2])


def test_fused_batch_follows_the_draw():
    cfg = MixConfig(0.4, 1.0)
    ds = DeviceImageDataset(IMGS, LABELS, DEV, augment=True, seed=5, mix=cfg)
    idx = torch.arange(40, 61)
    xr, yr = image_batch_reference(torch.as_tensor(IMGS), torch.as_tensor(LABELS), idx, 4, True, 5, 1, CIFAR_MEAN,
                                   CIFAR_STD)
    for no in range(4):
        p = draw_mix(cfg, 5, 1, 3, no, H, W)
        _check(ds.batch(idx.to(DEV), epoch=1, batch_no=no, rank=3), mix_reference(xr, yr, p), p.kind)


def test_without_a_mix_the_batch_kernel_is_unchanged():
    ds = DeviceImageDataset(IMGS, LABELS, DEV, augment=True, seed=5)
    idx = torch.arange(17)
    out = ds.batch(idx.to(DEV), epoch=3)
    assert len(out) == 2
    xr, yr = image_batch_reference(torch.as_tensor(IMGS), torch.as_tensor(LABELS), idx, 4, True, 5, 3, CIFAR_MEAN,
                                   CIFAR_STD)
    torch.testing.assert_close(out[0].cpu(), xr, atol=1e-6, rtol=0)
    assert torch.equal(out[1].cpu(), yr)


def _boxes(h, w):
    return [MixParams("mixup", 0.3), MixParams("cutmix", 1 - (h - 2) * 3 / (h * w), (2, h, 0, 3)),
            MixParams("cutmix", 1 - 4 * (w - 5) / (h * w), (0, 4, 5, w)), MixParams("cutmix", 0.0, (0, h, 0, w)),
            MixParams("cutmix", 1.0, (1, 1, 2, 2)), MixParams()]


# (5, 3, 9, 11): C H W no multiple of 4 (one element per thread); (3, 1, 17, 23) likewise, odd B; (2, 3, 32, 32):
# 16-byte pieces; (34, 3, 224, 224): 640k pairs of 16-byte pieces for the 2048 x 256 = 524k threads of one grid sweep
@pytest.mark.parametrize("shape", [(5, 3, 9, 11), (2, 3, 32, 32), (3, 1, 17, 23), (1, 3, 8, 8), (34, 3, 224, 224)])
def test_mix_batch_in_place(shape):
    B, _, h, w = shape
    g = torch.Generator().manual_seed(B)
    x = torch.randn(shape, generator=g)
    y = torch.randint(10, (B,), generator=g)
    for p in _boxes(h, w)[:2 if B == 34 else None]:
        xg, yg = x.to(DEV), y.to(DEV)
        yb, lam = torch.full_like(yg, -7), torch.full((1,), -7.0, device=DEV)
        got = mix_batch_(xg, yg, p, yb, lam)
        assert got[0] is xg and got[2] is yb and got[3] is lam
        _check(got, mix_reference(x, y, p), p.kind)
        if B % 2:
            assert torch.equal(xg[B // 2].cpu(), x[B // 2])
    got = mix_batch_(x.to(DEV), y.to(DEV), MixParams("mixup", 0.5))      # buffers of its own
    assert got[2].dtype == torch.int64 and got[3].shape == (1,) and float(got[3]) == 0.5


def test_mix_batch_on_a_batch_off_the_16_byte_grid():
    """C H W a multiple of 4 but the batch 4 bytes past a 16-byte boundary: the one-element path"""
    x = torch.randn(4, 3, 8, 8)
    y = torch.arange(4)
    buf = torch.empty(x.numel() + 1, device=DEV)
    xg = buf[1:].view(x.shape)
    xg.copy_(x)
    p = MixParams("cutmix", 1 - 12 / 64, (2, 5, 1, 5))
    _check(mix_batch_(xg, y.to(DEV), p), mix_reference(x, y, p), p.kind)


def test_refused_arguments():
    x, y = torch.randn(4, 3, 8, 8, device=DEV), torch.arange(4, device=DEV)
    with pytest.raises(ValueError, match="inside"):
        mix_batch_(x, y, MixParams("cutmix", 0.5, (0, 9, 0, 4)))
    with pytest.raises(ValueError, match="lam"):
        mix_batch_(x, y, MixParams("mixup", 1.5))
    with pytest.raises(RuntimeError, match="labels_b"):
        mix_batch_(x, y, MixParams("mixup", 0.5), labels_b=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="contiguous fp32"):
        mix_batch_(x.permute(0, 1, 3, 2), y, MixParams("mixup", 0.5))
