"""The segmentation augmentation kernel (csrc/kernels/seg_aug.hip) against the integer-coordinate reference of
data/seg_aug.py (itself tied to torch's grid_sample in tests/test_seg_aug_cpu.py).

The coordinates are integers on both sides, so the mask is compared bit for bit.  The image is three fp32 lerps of
sources in [0, 1]: at most 9 roundings of values <= 1, 9 * 2^-24 = 5.4e-7, so atol 1e-6 against the fp64 reference
(the bound tests/test_device_data.py uses); transforms whose coordinates are whole pixels are bit-exact."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seg_aug_cases as S
from deeplearning_mpi_amd.data import (DeviceSegDataset, SegAugConfig, SyntheticMasks, draw_seg_aug, seg_affine,
                                       seg_aug_reference)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-6
CASES = {**S.TRANSFORMS, **S.TIES}
NAMES = list(CASES)
MASK_FILL = {torch.float32: -1.0, torch.int64: -100}


def _native():
    from deeplearning_mpi_amd._ext import native

    return native()


def _run(images, masks, idx, table, Ho, Wo, image_fill, mask_fill, out=None):
    """One launch on outputs pre-filled with 7, so that an element the kernel did not write shows."""
    B, C = idx.numel(), images.shape[1]
    if out is None:
        out = (torch.empty(B, C, Ho, Wo, device=DEV), torch.empty(B, Ho, Wo, dtype=masks.dtype, device=DEV))
    out[0].fill_(7.0)
    out[1].fill_(7)
    _native().seg_aug_batch(images, masks, idx.to(DEV), table, image_fill, mask_fill, out[0], out[1])
    return out[0].cpu(), out[1].cpu()


@functools.lru_cache(maxsize=None)
def _fixed(shape, mask_dtype, image_fill):
    """Sources with one transform of CASES per sample, and the fp64 reference of all of them (computed once)."""
    C, H, W, Ho, Wo = shape
    images, masks = S.sources(len(NAMES), C, H, W, mask_dtype)
    table = S.table_of(CASES.values(), H, W, Ho, Wo)
    ref = seg_aug_reference(images, masks, torch.arange(len(NAMES)), table, Ho, Wo, image_fill, MASK_FILL[mask_dtype],
                            dtype=torch.float64)
    return images, masks, table, ref


# ------------------------------------------------------------------------------------------- fixed cases
@pytest.mark.parametrize("image_fill", [0.0, 0.25])
@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_fixed_cases(shape, mask_dtype, image_fill):
    C, H, W, Ho, Wo = shape
    images, masks, table, (ri, rm) = _fixed(shape, mask_dtype, image_fill)
    gi, gm, gt = images.to(DEV), masks.to(DEV), torch.from_numpy(table).to(DEV)
    n = len(NAMES)
    # B = 1: every transform alone; B = 5: five samples with five different rows, every row covered
    batches = [torch.tensor([i]) for i in range(n)] + [torch.arange(s, s + 5) for s in (0, 3, n - 5)]
    batches.append(torch.tensor([n - 1, 2, 6, 0, 4]))                      # ... and out of order
    for idx in batches:
        img, msk = _run(gi, gm, idx, gt, Ho, Wo, image_fill, MASK_FILL[mask_dtype])
        what = [NAMES[i] for i in idx.tolist()]
        assert msk.dtype == mask_dtype and torch.equal(msk, rm[idx]), what
        err = (img.double() - ri[idx]).abs().max().item()
        assert err <= ATOL, (what, err)
    out = NAMES.index("outside")
    assert (ri[out] == image_fill).all() and (rm[out] == MASK_FILL[mask_dtype]).all()


# -------------------------------------------------------------------------- identity and whole-pixel moves
@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("hw", [(16, 16), (17, 23)])
def test_identity_flips_and_quarter_turn_are_bit_exact(hw, mask_dtype):
    H, W = hw
    images, masks = S.sources(9, 3, H, W, mask_dtype)
    gi, gm = images.to(DEV), masks.to(DEV)
    ident = torch.from_numpy(S.table_of([{}] * 9, H, W, H, W)).to(DEV)
    idx = torch.tensor([4, 0, 8, 8, 1])
    img, msk = _run(gi, gm, idx, ident, H, W, 0.0, MASK_FILL[mask_dtype])
    assert torch.equal(img, images.index_select(0, idx)) and torch.equal(msk, masks.index_select(0, idx))
    moves = [dict(hflip=True), dict(vflip=True), dict(hflip=True, vflip=True), dict(tx=3, ty=-2), dict(degrees=180)]
    table = S.table_of(moves, H, W, H, W)
    idx = torch.arange(len(moves))
    img, msk = _run(gi, gm, idx, torch.from_numpy(np.concatenate([table, table[:4]])).to(DEV), H, W, 0.25,
                    MASK_FILL[mask_dtype])
    ri, rm = seg_aug_reference(images, masks, idx, np.concatenate([table, table[:4]]), H, W, 0.25,
                               MASK_FILL[mask_dtype])
    assert torch.equal(img, ri) and torch.equal(msk, rm)
    assert torch.equal(img[0], images[0].flip(-1)) and torch.equal(msk[1], masks[1].flip(-2))
    # a quarter turn into the transposed size
    turn = torch.from_numpy(S.table_of([dict(degrees=90)] * 9, H, W, W, H)).to(DEV)
    img, msk = _run(gi, gm, torch.tensor([2, 7]), turn, W, H, 0.0, MASK_FILL[mask_dtype])
    assert torch.equal(img, torch.rot90(images[[2, 7]], 1, (-2, -1)))
    assert torch.equal(msk, torch.rot90(masks[[2, 7]], 1, (-2, -1)))


# ------------------------------------------------------------------------------------ both store paths
@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.int64])
def test_store_paths_agree(mask_dtype):
    """Wo % 4 == 0 on 16-byte aligned outputs: 16-byte stores; Wo = 23, or an output (image or mask) that starts
    off the 16-byte grid: one column per thread.  The same samples give the same bits either way."""
    C, H, W = 3, 17, 23
    images, masks = S.sources(len(NAMES), C, H, W, mask_dtype)
    gi, gm = images.to(DEV), masks.to(DEV)
    idx = torch.tensor([5, 6, 1, 9, 10])
    fill = MASK_FILL[mask_dtype]
    for Ho, Wo in ((12, 20), (17, 23)):
        table = S.table_of(CASES.values(), H, W, Ho, Wo)
        ri, rm = seg_aug_reference(images, masks, idx, table, Ho, Wo, 0.25, fill, dtype=torch.float64)
        gt = torch.from_numpy(table).to(DEV)
        results = []
        for img_off, mask_off in ((0, 0), (1, 0), (0, 1), (1, 1)):       # elements past an aligned allocation
            xb = torch.empty(5 * C * Ho * Wo + 4, device=DEV)
            yb = torch.empty(5 * Ho * Wo + 2, dtype=mask_dtype, device=DEV)
            x = xb[img_off:img_off + 5 * C * Ho * Wo].view(5, C, Ho, Wo)
            y = yb[mask_off:mask_off + 5 * Ho * Wo].view(5, Ho, Wo)
            assert x.data_ptr() % 16 == 4 * img_off and y.data_ptr() % 16 == yb.element_size() * mask_off
            xb.fill_(3.0)
            yb.fill_(3)
            img, msk = _run(gi, gm, idx, gt, Ho, Wo, 0.25, fill, out=(x, y))
            assert torch.equal(msk, rm) and (img.double() - ri).abs().max().item() <= ATOL
            # nothing outside the views was written
            assert (xb[:img_off] == 3).all() and (xb[img_off + x.numel():] == 3).all()
            assert (yb[:mask_off] == 3).all() and (yb[mask_off + y.numel():] == 3).all()
            results.append(img)
        assert all(torch.equal(results[0], r) for r in results[1:])


# ------------------------------------------------------------------------------------- grid-stride wrap
@functools.lru_cache(maxsize=None)
def _large():
    g = torch.Generator().manual_seed(5)
    images = torch.rand(9, 3, 512, 512, generator=g)
    masks = torch.randint(5, (9, 512, 512), generator=g)
    return images, masks


def test_grid_stride_wrap_16_byte_path():
    """9 x 512 x 512 / 4 = 589,824 threads' worth of work against one sweep of 2048 x 256 = 524,288."""
    images, masks = _large()
    masks = masks.float()
    cfg = SegAugConfig(hflip=0.5, scale=(0.8, 1.25), rotate=30.0, translate=0.05)
    table = draw_seg_aug(cfg, 3, 0, 9, 512, 512, 512, 512)
    idx = torch.tensor([3, 1, 4, 0, 5, 8, 2, 6, 7])
    ri, rm = seg_aug_reference(images, masks, idx, table, 512, 512, 0.0, 0.0, dtype=torch.float64)
    img, msk = _run(images.to(DEV), masks.to(DEV), idx, torch.from_numpy(table).to(DEV), 512, 512, 0.0, 0.0)
    assert torch.equal(msk, rm)
    assert (img.double() - ri).abs().max().item() <= ATOL
    assert 0.02 < (rm != masks[idx]).float().mean() and (ri == 0).float().mean() < 0.5    # a real transform


def test_grid_stride_wrap_one_column_path():
    """3 x 300 x 601 = 540,900 one-column threads' worth against one sweep of 524,288; int64 masks."""
    images, masks = _large()
    cfg = SegAugConfig(vflip=0.5, scale=(0.8, 1.25), rotate=30.0, translate=0.05)
    table = draw_seg_aug(cfg, 4, 1, 9, 512, 512, 300, 601)
    idx = torch.tensor([8, 0, 5])
    ri, rm = seg_aug_reference(images, masks, idx, table, 300, 601, 0.5, -100, dtype=torch.float64)
    img, msk = _run(images.to(DEV), masks.to(DEV), idx, torch.from_numpy(table).to(DEV), 300, 601, 0.5, -100)
    assert torch.equal(msk, rm)
    assert (img.double() - ri).abs().max().item() <= ATOL


# ------------------------------------------------------------------------------------ following the draw
@pytest.mark.parametrize("K", [1, 3])
def test_dataset_follows_the_draw(K):
    cfg = SegAugConfig(hflip=0.5, vflip=0.3, scale=(0.7, 1.4), rotate=25.0, translate=0.1, prob=0.8, image_fill=0.5)
    src = SyntheticMasks(7, (3, 16, 20), seed=3, num_classes=K)
    fill = -100 if K > 1 else None
    ds = DeviceSegDataset(src, DEV, cfg, seed=11, out_size=(12, 16), mask_fill=fill)
    cpu = DeviceSegDataset(src, "cpu", cfg, seed=11, out_size=(12, 16), mask_fill=fill)
    assert ds.images.is_cuda and ds.masks.dtype == (torch.int64 if K > 1 else torch.float32)
    for epoch in (0, 1):
        table = draw_seg_aug(cfg, 11, epoch, 7, 16, 20, 12, 16)
        assert ds.table(epoch).dtype == torch.int32 and torch.equal(ds.table(epoch).cpu(), torch.from_numpy(table))
        idx = torch.tensor([5, 0, 3, 3, 6])
        got = ds.batch(idx.to(DEV), epoch)
        ri, rm = seg_aug_reference(cpu.images, cpu.masks, idx, table, 12, 16, 0.5, fill or 0.0, dtype=torch.float64)
        assert torch.equal(got["mask"].cpu(), rm) and (got["image"].cpu().double() - ri).abs().max().item() <= ATOL
        assert torch.equal(got["mask"].cpu(), cpu.batch(idx, epoch)["mask"])
        again = ds.batch(idx.to(DEV), epoch)                                # twice: identical bits
        assert torch.equal(again["image"], got["image"]) and torch.equal(again["mask"], got["mask"])
        solo = ds.batch(torch.tensor([3], device=DEV), epoch)              # whichever batch a sample is in
        other = ds.batch(torch.tensor([1, 2, 3, 4], device=DEV), epoch)
        assert torch.equal(solo["image"][0], got["image"][2]) and torch.equal(other["image"][2], got["image"][3])
        assert torch.equal(solo["mask"][0], got["mask"][2]) and torch.equal(other["mask"][2], got["mask"][3])
    assert ds.redraws == 2
    out = (torch.zeros(2, 3, 12, 16, device=DEV), torch.zeros(2, 12, 16, dtype=ds.masks.dtype, device=DEV))
    got = ds.batch(torch.tensor([1, 4], device=DEV), 1, out=out)
    assert got["image"] is out[0] and got["mask"] is out[1]
    assert torch.equal(out[0], ds.batch(torch.tensor([1, 4], device=DEV), 1)["image"])


# ------------------------------------------------------------------------------------------- fill values
def test_fill_values_of_a_sample_that_lands_outside():
    images, masks = S.sources(3, 2, 8, 12, torch.int64)
    table = S.table_of([{}, S.TRANSFORMS["outside"], dict(tx=0, ty=-9)], 8, 12, 8, 12)
    img, msk = _run(images.to(DEV), masks.to(DEV), torch.arange(3), torch.from_numpy(table).to(DEV), 8, 12, 0.25, -100)
    assert torch.equal(img[0], images[0]) and torch.equal(msk[0], masks[0])
    for b in (1, 2):
        assert (msk[b] == -100).all() and (img[b] == 0.25).all()


# ------------------------------------------------------------------------------------- refused arguments
def test_refused_arguments():
    f = _native().seg_aug_batch
    N, C, H, W, B = 4, 3, 8, 12, 2
    images, masks = (t.to(DEV) for t in S.sources(N, C, H, W))
    idx = torch.tensor([1, 3], device=DEV)
    table = torch.from_numpy(S.table_of([{}] * N, H, W, H, W)).to(DEV)
    out, om = torch.empty(B, C, H, W, device=DEV), torch.empty(B, H, W, device=DEV)
    f(images, masks, idx, table, 0.0, 0.0, out, om)
    f(images, masks.long(), idx, table, 0.0, 0.0, out, om.long())
    bad = [
        ("images must", dict(images=images.double())),
        ("images must", dict(images=images.cpu())),
        ("images must", dict(images=images[:, :, :, ::2])),
        ("images must", dict(images=images[0])),
        ("masks must", dict(masks=masks.int())),
        ("masks must", dict(masks=masks[:, :, :6].contiguous())),
        ("masks must", dict(masks=masks[:3])),
        ("masks must", dict(masks=masks.cpu())),
        ("idx must", dict(idx=idx.int())),
        ("idx must", dict(idx=idx.cpu())),
        ("idx must", dict(idx=idx[:0])),
        ("idx must", dict(idx=torch.arange(4, device=DEV)[::2])),
        ("table must", dict(table=table[:, :5].contiguous())),
        ("table must", dict(table=table[:3])),
        ("table must", dict(table=table.long())),
        ("table must", dict(table=table.t().contiguous().t())),
        ("out must", dict(out=out.double())),
        ("out must", dict(out=torch.empty(B + 1, C, H, W, device=DEV))),
        ("out must", dict(out=torch.empty(B, C + 1, H, W, device=DEV))),
        ("out must", dict(out=torch.empty(B, C, W, H, device=DEV).permute(0, 1, 3, 2))),
        ("out must", dict(out=torch.empty(B, C, H, 0, device=DEV))),
        ("out must", dict(out=out.cpu())),
        ("out_mask must", dict(om=om.long())),
        ("out_mask must", dict(om=torch.empty(B, H, W + 1, device=DEV))),
        ("out_mask must", dict(om=torch.empty(B, W, H, device=DEV).permute(0, 2, 1))),
        ("fill", dict(image_fill=float("nan"))),
    ]
    for match, kw in bad:
        a = dict(images=images, masks=masks, idx=idx, table=table, image_fill=0.0, mask_fill=0.0, out=out, om=om)
        a.update(kw)
        with pytest.raises(RuntimeError, match="seg_aug_batch: .*" + match):
            f(a["images"], a["masks"], a["idx"], a["table"], a["image_fill"], a["mask_fill"], a["out"], a["om"])
    ds = DeviceSegDataset(SyntheticMasks(4, (3, 8, 12)), DEV, SegAugConfig(hflip=0.5))
    with pytest.raises(ValueError, match="out must"):      # the dataset knows its output size: another is refused
        ds.batch(idx, 0, out=(torch.empty(B, C, H + 1, W, device=DEV), torch.empty(B, H + 1, W, device=DEV)))
    with pytest.raises(ValueError, match="out must"):
        ds.batch(idx, 0, out=(out, torch.empty(B, H + 1, W, device=DEV)))
    with pytest.raises(RuntimeError, match="out_mask must"):
        ds.batch(idx, 0, out=(out, om.long()))
    with pytest.raises(RuntimeError, match="out must"):
        ds.batch(idx, 0, out=(torch.empty(B, C, W, H, device=DEV).permute(0, 1, 3, 2), om))
    with pytest.raises(ValueError, match="Q16"):
        seg_affine(H, W, H, W, scale=1e-6)


# ------------------------------------------------------------------------------------ the trainer on the GPU
def test_trainer_eager_and_captured_steps_agree(tmp_path):
    """--graph 0 and --graph 1 see the same augmented batches (the batch kernel runs outside the captured step
    and writes its inputs in place) and draw one table per epoch: nothing else crosses from the host per step.
    Set size 8 is the CPU test's case (one full batch per epoch: the step is never replayed); 24 gives four full
    batches per epoch, of which six are replays."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "seg_aug_trainer_child.py"), "8", "24"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    runs = {(j["size"], j["graph"]): j for j in (json.loads(ln) for ln in r.stdout.splitlines()
                                                  if ln.startswith("{") and '"redraws"' in ln)}
    assert sorted(runs) == [(8, 0), (8, 1), (24, 0), (24, 1)]
    for size, batches, full, replays in ((8, 4, 2, 0), (24, 10, 8, 6)):
        eager, graph = runs[size, 0], runs[size, 1]
        for j in (eager, graph):
            assert j["dataset"] == "DeviceSegDataset" and j["device"] == "cuda"
            assert j["redraws"] == 2 and j["batches"] == batches          # one table per epoch, none per step
            assert len(j["loss"]) == 2 and np.isfinite(j["loss"]).all()
        assert eager["in_place"] == 0 and eager["replays"] == 0
        assert graph["in_place"] == full and graph["replays"] == replays
        assert eager["loss"] == graph["loss"], (size, eager["loss"], graph["loss"])
