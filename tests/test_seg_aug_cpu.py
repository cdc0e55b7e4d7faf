"""Segmentation augmentation on the CPU (data/seg_aug.py): the draw of the epoch's table, the integer-coordinate
reference against torch's grid_sample in fp64, the cases that must be bit-exact, the nearest rule at ties,
DeviceSegDataset on a CPU device and the trainer's --aug_* flags."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_aug_cases as S
from deeplearning_mpi_amd.data import (DeviceBatches, DeviceCachedDataset, DeviceSegDataset, SegAugConfig,
                                       SyntheticMasks, draw_seg_aug, draw_seg_params, seg_affine, seg_aug_reference)

FULL = SegAugConfig(hflip=0.5, vflip=0.3, scale=(0.7, 1.4), rotate=25.0, translate=0.1, prob=0.8)
IDENTITY = [65536, 0, 0, 0, 65536, 0]


# ------------------------------------------------------------------------------------------- the draw
def test_draw_is_a_function_of_seed_and_epoch():
    a = draw_seg_aug(FULL, 7, 3, 40, 17, 23, 17, 23)
    assert a.dtype == np.int32 and a.shape == (40, 6)
    assert np.array_equal(a, draw_seg_aug(FULL, 7, 3, 40, 17, 23, 17, 23))
    assert not np.array_equal(a, draw_seg_aug(FULL, 7, 4, 40, 17, 23, 17, 23))
    assert not np.array_equal(a, draw_seg_aug(FULL, 8, 3, 40, 17, 23, 17, 23))
    # the [N, 7] block of uniforms fills row by row: row i is the same for every N > i
    assert np.array_equal(a[:11], draw_seg_aug(FULL, 7, 3, 11, 17, 23, 17, 23))
    # the stream does not depend on the config: the flips of two configs with the same probabilities agree
    p = draw_seg_params(FULL, 7, 3, 40, 17, 23)
    q = draw_seg_params(SegAugConfig(hflip=0.5, vflip=0.3), 7, 3, 40, 17, 23)
    assert np.array_equal(p["hflip"], q["hflip"]) and np.array_equal(p["vflip"], q["vflip"])
    assert 0 < p["hflip"].sum() < 40


def test_prob_0_without_flips_is_the_identity():
    cfg = SegAugConfig(scale=(0.5, 2.0), rotate=45.0, translate=0.2, prob=0.0)
    assert cfg.enabled
    t = draw_seg_aug(cfg, 1, 0, 9, 12, 20, 12, 20)
    assert (t == np.array(IDENTITY, dtype=np.int32)).all()
    assert (draw_seg_aug(SegAugConfig(), 1, 0, 9, 12, 20, 12, 20) == np.array(IDENTITY)).all()
    # prob < 1 keeps the flips of the samples it leaves alone
    p = draw_seg_params(SegAugConfig(hflip=1.0, rotate=45.0, prob=0.0), 1, 0, 9, 12, 20)
    assert p["hflip"].all() and (p["degrees"] == 0).all() and (p["scale"] == 1).all()


def test_drawn_parameters_lie_in_their_ranges():
    H, W, N = 30, 50, 4000
    p = draw_seg_params(FULL, 0, 0, N, H, W)
    on = p["degrees"] != 0
    assert 0.75 < on.mean() < 0.85                                          # prob = 0.8
    assert (p["scale"][on] >= 0.7).all() and (p["scale"][on] <= 1.4).all()
    assert p["scale"][on].min() < 0.72 and p["scale"][on].max() > 1.37       # ... and fill them
    assert abs(np.log(p["scale"][on]).mean()) < 0.03                         # log-uniform about 1
    assert (np.abs(p["degrees"]) <= 25).all() and np.abs(p["degrees"]).max() > 24.5
    assert (np.abs(p["tx"]) <= 0.1 * W).all() and np.abs(p["tx"]).max() > 0.098 * W
    assert (np.abs(p["ty"]) <= 0.1 * H).all() and np.abs(p["ty"]).max() > 0.098 * H
    assert (p["scale"][~on] == 1).all() and (p["tx"][~on] == 0).all() and (p["ty"][~on] == 0).all()
    assert 0.45 < p["hflip"].mean() < 0.55 and 0.25 < p["vflip"].mean() < 0.35


def test_config_validation():
    assert not SegAugConfig().enabled
    for kw in (dict(hflip=0.5), dict(vflip=1.0), dict(scale=(0.9, 1.1)), dict(rotate=10.0), dict(translate=0.1),
               dict(prob=0.5), dict(image_fill=0.5)):
        assert SegAugConfig(**kw).enabled, kw
    assert SegAugConfig(scale=[1, 2]).scale == (1.0, 2.0)
    for kw in (dict(hflip=-0.1), dict(hflip=1.5), dict(vflip=2), dict(prob=-1), dict(prob=float("nan")),
               dict(scale=(0.0, 1.0)), dict(scale=(1.2, 1.1)), dict(scale=(1.0, float("inf"))), dict(scale=1.0),
               dict(scale=(1.0, 2.0, 3.0)), dict(rotate=-1.0), dict(rotate=float("nan")), dict(translate=-0.1),
               dict(translate=float("inf")), dict(image_fill=float("nan"))):
        with pytest.raises(ValueError):
            SegAugConfig(**kw)
    with pytest.raises(ValueError, match="Q16"):
        seg_affine(8, 8, 8, 8, scale=1e-5)            # a = 1e5 source pixels per output pixel
    with pytest.raises(ValueError, match="Q16"):
        seg_affine(8, 8, 8, 8, tx=40000)
    with pytest.raises(ValueError):
        seg_affine(8, 8, 8, 8, scale=0.0)
    with pytest.raises(ValueError):
        seg_affine(8, 8, 0, 8)
    assert seg_affine(17, 23, 17, 23) == tuple(IDENTITY)
    assert seg_affine(17, 23, 17, 23, hflip=True) == (-65536, 0, 22 * 65536, 0, 65536, 0)
    assert seg_affine(17, 23, 9, 11) == (65536, 0, 6 * 65536, 0, 65536, 4 * 65536)     # the centre crop


# ------------------------------------------------------------------- the reference against grid_sample
def _coords(row, Ho, Wo):
    a, b, c, d, e, f = (int(v) for v in row)
    xs = torch.arange(Wo, dtype=torch.int64).view(1, Wo)
    ys = torch.arange(Ho, dtype=torch.int64).view(Ho, 1)
    return a * xs + b * ys + c, d * xs + e * ys + f


@pytest.mark.parametrize("shape", S.SHAPES)
def test_reference_matches_grid_sample_in_fp64(shape):
    C, H, W, Ho, Wo = shape
    names = list(S.TRANSFORMS)
    table = S.table_of(S.TRANSFORMS.values(), H, W, Ho, Wo)
    images, masks = S.sources(len(names), C, H, W)
    idx = torch.arange(len(names))
    img, msk = seg_aug_reference(images, masks, idx, table, Ho, Wo, 0.0, 0.0, dtype=torch.float64)
    assert img.dtype == torch.float64 and img.shape == (len(names), C, Ho, Wo) and msk.dtype == torch.float32
    ties = 0
    for i, name in enumerate(names):
        X, Y = _coords(table[i], Ho, Wo)
        grid = torch.stack([(2 * (X.double() / 65536) + 1) / W - 1, (2 * (Y.double() / 65536) + 1) / H - 1], -1)[None]
        want = F.grid_sample(images[i:i + 1].double(), grid, mode="bilinear", padding_mode="zeros",
                             align_corners=False)
        assert (img[i] - want[0]).abs().max().item() <= 1e-12, name
        near = F.grid_sample(masks[i:i + 1, None].double(), grid, mode="nearest", padding_mode="zeros",
                             align_corners=False)[0, 0]
        tie = ((X & 0xFFFF) == 0x8000) | ((Y & 0xFFFF) == 0x8000)     # grid_sample: to even; here: up
        ties += int(tie.sum())
        assert torch.equal(msk[i].double()[~tie], near[~tie]), name
    assert ties == 0
    assert (msk[names.index("outside")] == 0).all() and (img[names.index("outside")] == 0).all()
    # the fp32 path rounds three lerps of values <= 1
    img32, msk32 = seg_aug_reference(images, masks, idx, table, Ho, Wo, 0.0, 0.0)
    assert img32.dtype == torch.float32 and torch.equal(msk32, msk)
    assert (img32.double() - img).abs().max().item() <= 9 * 2.0 ** -24


# --------------------------------------------------------------------------------- bit-exact cases
def _one(images, masks, H, W, Ho, Wo, image_fill=0.25, mask_fill=-1.0, **t):
    table = np.repeat(S.table_of([t], H, W, Ho, Wo), images.shape[0], 0)
    return seg_aug_reference(images, masks, torch.arange(images.shape[0]), table, Ho, Wo, image_fill, mask_fill)


@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("shape", [(3, 17, 23), (1, 8, 12)])
def test_flips_shift_and_quarter_turn_are_exact(shape, mask_dtype):
    C, H, W = shape
    images, masks = S.sources(2, C, H, W, mask_dtype)
    for t, dims in ((dict(), ()), (dict(hflip=True), (-1,)), (dict(vflip=True), (-2,)),
                    (dict(hflip=True, vflip=True), (-2, -1))):
        img, msk = _one(images, masks, H, W, H, W, **t)
        assert torch.equal(img, images.flip(dims)) and torch.equal(msk, masks.flip(dims)), t
        assert msk.dtype == mask_dtype
    # x_src = x + 3, y_src = y - 2: rows 2.. of the output hold rows ..H-2 of the source, columns ..W-3 columns 3..
    img, msk = _one(images, masks, H, W, H, W, tx=3, ty=-2)
    wi, wm = torch.full_like(images, 0.25), torch.full_like(masks, -1)
    wi[:, :, 2:, :W - 3] = images[:, :, :H - 2, 3:]
    wm[:, 2:, :W - 3] = masks[:, :H - 2, 3:]
    assert torch.equal(img, wi) and torch.equal(msk, wm)
    # a quarter turn into the transposed size is torch.rot90
    img, msk = _one(images, masks, H, W, W, H, degrees=90)
    assert torch.equal(img, torch.rot90(images, 1, (-2, -1))) and torch.equal(msk, torch.rot90(masks, 1, (-2, -1)))
    img, msk = _one(images, masks, H, W, W, H, degrees=-90)
    assert torch.equal(img, torch.rot90(images, -1, (-2, -1))) and torch.equal(msk, torch.rot90(masks, -1, (-2, -1)))
    img, msk = _one(images, masks, H, W, H, W, degrees=180)
    assert torch.equal(img, images.flip((-2, -1))) and torch.equal(msk, masks.flip((-2, -1)))


def test_quarter_turn_of_a_square():
    images, masks = S.sources(2, 2, 16, 16)
    img, msk = _one(images, masks, 16, 16, 16, 16, degrees=90)
    assert torch.equal(img, torch.rot90(images, 1, (-2, -1))) and torch.equal(msk, torch.rot90(masks, 1, (-2, -1)))


GRID = torch.arange(16.0).view(1, 1, 4, 4)      # pixel (y, x) holds 4 y + x
FM = -1.0                                       # mask_fill


def test_ties_round_up_by_hand():
    """Coordinates on .5 exactly, on the 4 x 4 image whose pixel (y, x) holds 4 y + x (image_fill 0, mask_fill -1).
    Nearest takes the HIGHER neighbour; round-half-to-even would take 0, 2, 4 for 0.5, 2.5, 4.5."""
    images, masks = GRID, GRID[0]
    # translation (0.5, 0.5): x_src = x + 0.5 -> the mask of (y + 1, x + 1); the image the mean of the 2 x 2 block
    img, msk = _one(images, masks, 4, 4, 4, 4, 0.0, FM, **S.TIES["half_shift"])
    assert msk[0].tolist() == [[5, 6, 7, FM], [9, 10, 11, FM], [13, 14, 15, FM], [FM, FM, FM, FM]]
    assert img[0, 0].tolist() == [[2.5, 3.5, 4.5, 2.5], [6.5, 7.5, 8.5, 4.5], [10.5, 11.5, 12.5, 6.5],
                                  [6.25, 6.75, 7.25, 3.75]]
    # s = 0.5: x_src = 2 x - 1.5 = -1.5, 0.5, 2.5, 4.5 -> nearest -1, 1, 3, 5
    img, msk = _one(images, masks, 4, 4, 4, 4, 0.0, FM, **S.TIES["half"])
    assert msk[0].tolist() == [[FM, FM, FM, FM], [FM, 5, 7, FM], [FM, 13, 15, FM], [FM, FM, FM, FM]]
    assert img[0, 0].tolist() == [[0, 0, 0, 0], [0, 2.5, 4.5, 0], [0, 10.5, 12.5, 0], [0, 0, 0, 0]]
    # s = 2 into 5 x 5: x_src = x / 2 + 0.5 = 0.5, 1, 1.5, 2, 2.5 -> nearest 1, 1, 2, 2, 3; the image is linear, so
    # its bilinear value is 4 y_src + x_src = 2 y + x / 2 + 2.5
    img, msk = _one(images, masks, 4, 4, 5, 5, 0.0, FM, **S.TIES["double"])
    assert msk[0].tolist() == [[5, 5, 6, 6, 7], [5, 5, 6, 6, 7], [9, 9, 10, 10, 11], [9, 9, 10, 10, 11],
                               [13, 13, 14, 14, 15]]
    assert img[0, 0].tolist() == [[2 * y + x / 2 + 2.5 for x in range(5)] for y in range(5)]
    row = seg_affine(4, 4, 5, 5, **S.TIES["double"])
    assert row == (32768, 0, 32768, 0, 32768, 32768)


# ---------------------------------------------------------------------------------- the dataset on the CPU
@pytest.mark.parametrize("K", [1, 3])
def test_dataset_follows_the_table_on_the_cpu(K):
    src = SyntheticMasks(7, (3, 16, 20), seed=3, num_classes=K)
    ds = DeviceSegDataset(src, "cpu", FULL, seed=11, out_size=(12, 16), mask_fill=-100 if K > 1 else None)
    cached = DeviceCachedDataset(src, "cpu")
    images, masks = cached.fields
    assert len(ds) == 7 and ds.masks.dtype == masks.dtype
    for epoch in (0, 1):
        table = draw_seg_aug(FULL, 11, epoch, 7, 16, 20, 12, 16)
        assert torch.equal(ds.table(epoch), torch.from_numpy(table))
        idx = torch.tensor([5, 0, 3, 3, 6])
        got = ds.batch(idx, epoch)
        wi, wm = seg_aug_reference(images, masks, idx, table, 12, 16, 0.0, -100 if K > 1 else 0.0)
        assert torch.equal(got["image"], wi) and torch.equal(got["mask"], wm)
        assert got["image"].shape == (5, 3, 12, 16) and got["mask"].dtype == masks.dtype
        # a sample does not depend on the batch it is in
        solo = ds.batch(torch.tensor([3]), epoch)
        other = ds.batch(torch.tensor([1, 2, 3]), epoch)
        assert torch.equal(solo["image"][0], got["image"][2]) and torch.equal(other["image"][2], got["image"][3])
        assert torch.equal(solo["mask"][0], got["mask"][2]) and torch.equal(other["mask"][2], got["mask"][3])
    assert ds.redraws == 2                         # one table per epoch, however many batches
    out = (torch.zeros(2, 3, 12, 16), torch.zeros(2, 12, 16, dtype=masks.dtype))
    got = ds.batch(torch.tensor([1, 4]), 1, out=out)
    assert got["image"] is out[0] and got["mask"] is out[1] and out[0].abs().sum() > 0
    with pytest.raises(ValueError, match="out"):
        ds.batch(torch.tensor([1, 4]), 1, out=(out[0][:, :, :8], out[1]))


def test_identity_config_equals_the_cached_dataset():
    for K in (1, 4):
        src = SyntheticMasks(6, (3, 16, 16), seed=1, num_classes=K)
        ds = DeviceSegDataset(src, "cpu", SegAugConfig(), mask_fill=-100 if K > 1 else None)
        cached = DeviceCachedDataset(src, "cpu")
        for a, b in zip(DeviceBatches(ds, 4), DeviceBatches(cached, 4)):
            assert list(a) == ["image", "mask"] == list(b)
            assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask"], b["mask"])
            assert a["mask"].dtype == b["mask"].dtype


def test_dataset_arguments():
    with pytest.raises(ValueError, match="mask_fill"):
        DeviceSegDataset(SyntheticMasks(2, (3, 8, 8), num_classes=3), "cpu", FULL)       # int64 masks: no default
    with pytest.raises(ValueError, match="mask_fill"):
        DeviceSegDataset(SyntheticMasks(2, (3, 8, 8), num_classes=3), "cpu", FULL, mask_fill=0.5)
    with pytest.raises(ValueError, match="out_size"):
        DeviceSegDataset(SyntheticMasks(2, (3, 8, 8)), "cpu", FULL, out_size=(0, 8))
    with pytest.raises(TypeError):
        DeviceSegDataset(SyntheticMasks(2, (3, 8, 8)), "cpu", None)
    with pytest.raises(ValueError, match="image"):
        DeviceSegDataset([torch.zeros(3, 8, 8)], "cpu", FULL)
    assert DeviceSegDataset(SyntheticMasks(2, (3, 8, 8)), "cpu", FULL).mask_fill == 0.0


# ----------------------------------------------------------------------------------------- the trainer
BASE = ["--device", "cpu", "--backend", "gloo", "--synthetic", "--synthetic_size", "8", "--image_size", "32",
        "--batch_size", "4", "--num_epochs", "2", "--workers", "0", "--eval_every", "100"]
AUG = ["--aug_hflip", "0.5", "--aug_vflip", "0.5", "--aug_scale", "0.8", "1.25", "--aug_rotate", "20",
       "--aug_translate", "0.1"]


def _train(tmp_path, extra):
    from deeplearning_mpi_amd.apps import segmentation as seg

    args = seg.parse_args(BASE + ["--log_dir", str(tmp_path / "logs"), "--model_dir", str(tmp_path)] + extra)
    return seg.run(args)["loss"]


@pytest.mark.parametrize("K", [1, 3])
def test_trainer_with_augmentation_on_the_cpu(tmp_path, K):
    k = ["--num_classes", str(K)]
    plain, aug, again = _train(tmp_path, k), _train(tmp_path, k + AUG), _train(tmp_path, k + AUG)
    assert len(aug) == 2 and np.isfinite(aug).all() and np.isfinite(plain).all()
    assert aug == again                                   # the draw is a function of (seed, epoch, index)
    assert aug != plain


def test_trainer_flags(capsys):
    from deeplearning_mpi_amd.apps import segmentation as seg

    args = seg.parse_args(BASE + ["--data_on_device", "1"])
    assert (args.aug_hflip, args.aug_vflip, args.aug_prob, args.aug_scale, args.aug_rotate, args.aug_translate) == \
        (0.0, 0.0, 1.0, [1.0, 1.0], 0.0, 0.0)
    assert not seg.seg_aug_config(args).enabled
    train, test, _ = seg.build_data_loaders(args, torch.device("cpu"))
    assert type(train.ds) is DeviceCachedDataset and type(test.ds) is DeviceCachedDataset
    args = seg.parse_args(BASE + AUG + ["--num_classes", "3", "--ignore_index", "-7", "--random_seed", "5"])
    cfg = seg.seg_aug_config(args)
    assert cfg == SegAugConfig(hflip=0.5, vflip=0.5, scale=(0.8, 1.25), rotate=20.0, translate=0.1)
    train, test, _ = seg.build_data_loaders(args, torch.device("cpu"))
    assert type(train.ds) is DeviceSegDataset and type(test.ds) is DeviceCachedDataset
    assert train.ds.mask_fill == -7 and train.ds.seed == 5 and train.ds.aug == cfg and len(train.ds) == 6
    for bad in (AUG + ["--data_on_device", "0"], ["--aug_hflip", "1.5"], ["--aug_scale", "2", "1"],
                ["--aug_rotate", "-3"]):
        with pytest.raises(SystemExit):
            seg.parse_args(BASE + bad)
        assert "--aug_" in capsys.readouterr().err
    args = seg.build_argparser().parse_args(BASE + AUG + ["--data_on_device", "0"])      # (unchecked namespace)
    with pytest.raises(ValueError, match="data_on_device"):
        seg.build_data_loaders(args, torch.device("cpu"))
