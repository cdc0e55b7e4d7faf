"""Elastic deformation on the CPU (data/seg_aug.py): the axis tables, the integer B-spline field against the plain
fp64 formula, the lattices' draw, the reference with a lattice, and the trainer's flags."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_aug_cases as S
from deeplearning_mpi_amd.data import (DeviceCachedDataset, DeviceSegDataset, SegAugConfig, draw_seg_aug,
                                       draw_seg_elastic, seg_aug_reference, seg_elastic_axis, seg_elastic_field)
from deeplearning_mpi_amd.data import seg_aug as SA

MOVES = [{}, dict(hflip=True), dict(scale=1.3, degrees=30, tx=1.7, ty=-2.2), dict(vflip=True, scale=0.77, degrees=-17)]


def _basis(n, G):
    """Cell and the four cubic B-spline basis values of every pixel centre, in fp64."""
    u = (np.arange(n) + 0.5) * G / n
    i = np.floor(u)
    t = u - i
    return i.astype(np.int64), np.stack([(1 - t) ** 3, 3 * t ** 3 - 6 * t ** 2 + 4,
                                         -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3], 1) / 6


@pytest.mark.parametrize("n,G", [(7, 1), (136, 3), (33, 32)])
def test_axis_table(n, G):
    e = seg_elastic_axis(n, G)
    i, basis = _basis(n, G)
    assert e.dtype == np.int32 and e.shape == (n, 5)
    assert (e[:, 1:] >= 0).all() and (e[:, 1:].astype(np.int64).sum(1) == 2 ** 20).all()
    assert np.array_equal(e[:, 0], i) and e[:, 0].min() >= 0 and e[:, 0].max() <= G - 1
    assert np.abs(e[:, 1:] / 2.0 ** 20 - basis).max() <= 2.0 ** -19


@pytest.mark.parametrize("sigma", [8.0, 1024.0])
@pytest.mark.parametrize("Ho,Wo,G", [(33, 136, 3), (5, 4, 1), (40, 36, 32)])
def test_integer_field_against_the_fp64_spline(Ho, Wo, G, sigma):
    """The direct 16-term sum with unrounded weights.  Each axis' weights are off by <= 2^-18 in total after the
    sum fix-up, and each pass rounds once (2^-17 px): max|D| 2^-17 + 2^-15 px; a wrong index is off by ~D."""
    D = draw_seg_elastic(SegAugConfig(elastic_sigma=sigma, elastic_grid=G), 3, 1, 4)
    got = seg_elastic_field(D, seg_elastic_axis(Wo, G), seg_elastic_axis(Ho, G)).numpy() / 65536.0
    (ix, bx), (iy, by) = _basis(Wo, G), _basis(Ho, G)
    Df = D / 65536.0
    win = Df[:, :, (iy[:, None] + np.arange(4))[:, :, None, None], (ix[:, None] + np.arange(4))[None, None]]
    want = np.einsum("yb,xa,ncybxa->ncyx", by, bx, win)
    assert got.shape == (4, 2, Ho, Wo) and np.abs(got).max() <= np.abs(Df).max()
    assert np.abs(got - want).max() <= np.abs(Df).max() * 2.0 ** -17 + 2.0 ** -15
    assert np.abs(want).max() > 0.1 * sigma                       # a real field


def test_zero_and_constant_lattices_are_bit_exact():
    C, H, W, Ho, Wo, G = 3, 17, 23, 12, 20, 3
    images, masks = S.sources(4, C, H, W, torch.int64)
    table, idx = S.table_of(MOVES, H, W, Ho, Wo), torch.tensor([2, 0, 3, 3, 1])
    plain = seg_aug_reference(images, masks, idx, table, Ho, Wo, 0.25, -100)
    zero = seg_aug_reference(images, masks, idx, table, Ho, Wo, 0.25, -100, lattice=np.zeros((4, 2, 6, 6), np.int32))
    assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1])
    lat = np.zeros((4, 2, G + 3, G + 3), np.int32)
    lat[:, 0], lat[:, 1] = 3 * 65536, -2 * 65536                  # k = (3, -2) whole pixels
    moved = table.copy()
    moved[:, 2] += 3 * 65536
    moved[:, 5] -= 2 * 65536
    const = seg_aug_reference(images, masks, idx, table, Ho, Wo, 0.25, -100, lattice=lat, grid=G)
    want = seg_aug_reference(images, masks, idx, moved, Ho, Wo, 0.25, -100)
    assert torch.equal(const[0], want[0]) and torch.equal(const[1], want[1])
    assert not torch.equal(const[1], plain[1])
    with pytest.raises(ValueError, match="lattice"):
        seg_aug_reference(images, masks, idx, table, Ho, Wo, lattice=lat, grid=4)


@pytest.mark.parametrize("Ho,Wo,G", [(17, 23, 3), (9, 11, 1)])
def test_reference_with_a_lattice_matches_grid_sample_in_fp64(Ho, Wo, G):
    C, H, W = 2, 17, 23
    images, masks = S.sources(4, C, H, W)
    table = S.table_of(MOVES, H, W, Ho, Wo)
    lat = draw_seg_elastic(SegAugConfig(elastic_sigma=4.0, elastic_grid=G), 5, 0, 4)
    img, _ = seg_aug_reference(images, masks, torch.arange(4), table, Ho, Wo, dtype=torch.float64, lattice=lat, grid=G)
    field = seg_elastic_field(lat, seg_elastic_axis(Wo, G), seg_elastic_axis(Ho, G))
    xs, ys = torch.arange(Wo).view(1, Wo), torch.arange(Ho).view(Ho, 1)
    for i, (a, b, c, d, e, f) in enumerate(table.astype(np.int64).tolist()):
        X, Y = a * xs + b * ys + c + field[i, 0], d * xs + e * ys + f + field[i, 1]
        grid = torch.stack([(2 * (X.double() / 65536) + 1) / W - 1, (2 * (Y.double() / 65536) + 1) / H - 1], -1)[None]
        want = F.grid_sample(images[i:i + 1].double(), grid, mode="bilinear", padding_mode="zeros",
                             align_corners=False)
        assert (img[i] - want[0]).abs().max().item() <= 1e-12, i


def test_draw():
    cfg = SegAugConfig(elastic_sigma=8.0, elastic_grid=5, elastic_prob=0.6)
    a, b = draw_seg_elastic(cfg, 7, 3, 5), draw_seg_elastic(cfg, 7, 3, 9)
    assert a.dtype == np.int32 and a.shape == (5, 2, 8, 8) and np.array_equal(a, b[:5])
    dropped = (b == 0).all(axis=(1, 2, 3))
    assert 0 < dropped.sum() < 9 and np.abs(b).max() <= 4 * 8.0 * 65536
    assert not any(np.array_equal(b, draw_seg_elastic(cfg, s, e, 9)) for s, e in ((7, 4), (8, 3)))
    assert not draw_seg_elastic(SegAugConfig(elastic_sigma=8.0, elastic_prob=0.0), 7, 3, 9).any()
    assert not draw_seg_elastic(SegAugConfig(elastic_grid=5), 7, 3, 9).any()
    full = SegAugConfig(hflip=0.5, scale=(0.8, 1.25), rotate=20.0, translate=0.1)
    both = SegAugConfig(hflip=0.5, scale=(0.8, 1.25), rotate=20.0, translate=0.1, elastic_sigma=8.0, elastic_grid=5)
    assert np.array_equal(draw_seg_aug(full, 7, 3, 9, 17, 23, 17, 23), draw_seg_aug(both, 7, 3, 9, 17, 23, 17, 23))
    for bad in (dict(elastic_sigma=-1.0), dict(elastic_sigma=1025.0), dict(elastic_grid=0), dict(elastic_grid=33),
                dict(elastic_grid=2.5), dict(elastic_prob=1.5)):
        with pytest.raises(ValueError, match="elastic"):
            SegAugConfig(**bad)


BASE = ["--device", "cpu", "--backend", "gloo", "--synthetic", "--synthetic_size", "8", "--image_size", "32",
        "--batch_size", "4", "--num_epochs", "2", "--workers", "0", "--eval_every", "100"]


def test_trainer_flags_and_two_steps(tmp_path, monkeypatch, capsys):
    from deeplearning_mpi_amd.apps import segmentation as seg

    calls = []
    field = SA.seg_elastic_field
    monkeypatch.setattr(SA, "seg_elastic_field", lambda *a: calls.append(1) or field(*a))
    out = ["--log_dir", str(tmp_path / "logs"), "--model_dir", str(tmp_path)]
    args = seg.parse_args(BASE + out + ["--data_on_device", "1"])
    assert (args.aug_elastic_sigma, args.aug_elastic_grid, args.aug_elastic_prob) == (0.0, 3, 1.0)
    assert type(seg.build_data_loaders(args, torch.device("cpu"))[0].ds) is DeviceCachedDataset
    args = seg.parse_args(BASE + out + ["--aug_hflip", "0.5"])
    train = seg.build_data_loaders(args, torch.device("cpu"))[0]
    assert type(train.ds) is DeviceSegDataset and not train.ds.elastic and train.ds._lattice is None
    assert np.isfinite(seg.run(args)["loss"]).all() and not calls          # the affine path never meets the field
    args = seg.parse_args(BASE + out + ["--aug_elastic_sigma", "4", "--aug_elastic_grid", "2"])
    assert seg.seg_aug_config(args) == SegAugConfig(elastic_sigma=4.0, elastic_grid=2)
    loss = seg.run(args)["loss"]
    assert len(loss) == 2 and np.isfinite(loss).all() and len(calls) == 4   # 6 training pairs: batches of 4 and 2
    for bad in (["--aug_elastic_sigma", "4", "--data_on_device", "0"], ["--aug_elastic_grid", "40"]):
        with pytest.raises(SystemExit):
            seg.parse_args(BASE + bad)
        assert "--aug_" in capsys.readouterr().err
