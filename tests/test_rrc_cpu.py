"""RandomResizedCrop on the CPU (data/rrc.py): the draw of the epoch's crop table, the box rule, the anti-aliased
resampling of rrc_reference against torch's own in fp64, the classification trainer on .npy arrays, and the
converter that writes them."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import rrc_cases as R
import torch

from deeplearning_mpi_amd.data import (DeviceImageDataset, RrcConfig, center_box, draw_rrc, image_batch_reference,
                                       rrc_reference, rrc_taps, rrc_weights)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------- the table ---------------------------------------------------
def test_table_depends_on_seed_epoch_and_index_alone():
    cfg = RrcConfig()
    a = draw_rrc(cfg, 7, 3, 50, 40, 48)
    assert a.dtype == np.int32 and a.shape == (50, 5) and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(a, draw_rrc(cfg, 7, 3, 50, 40, 48))                 # repeats across calls
    assert not np.array_equal(a, draw_rrc(cfg, 7, 4, 50, 40, 48))             # another epoch
    assert not np.array_equal(a, draw_rrc(cfg, 8, 3, 50, 40, 48))             # another seed
    assert np.array_equal(a[:13], draw_rrc(cfg, 7, 3, 13, 40, 48))            # row i does not depend on N
    assert 5 < a[:, 4].sum() < 45                                             # both flips occur
    assert (draw_rrc(RrcConfig(hflip=0.0), 7, 3, 50, 40, 48)[:, 4] == 0).all()
    # the flip does not move the boxes: one block of uniforms, always drawn whole
    assert np.array_equal(a[:, :4], draw_rrc(RrcConfig(hflip=0.0), 7, 3, 50, 40, 48)[:, :4])


@pytest.mark.parametrize("H,W", [(40, 48), (32, 32), (7, 120), (1, 1)])
def test_every_box_lies_inside_the_image(H, W):
    for cfg in (RrcConfig(), RrcConfig(scale=(0.5, 1.0), ratio=(0.3, 3.0)), RrcConfig(scale=(1.0, 1.0))):
        top, left, h, w, flip = draw_rrc(cfg, 1, 0, 300, H, W).T
        assert (h >= 1).all() and (w >= 1).all() and (top >= 0).all() and (left >= 0).all()
        assert (top + h <= H).all() and (left + w <= W).all() and set(flip) <= {0, 1}


def test_dataset_batches_do_not_depend_on_batch_composition():
    data, labels = R.source(20, 24, N=12)
    ds = DeviceImageDataset(data, labels, "cpu", rrc=RrcConfig(), out_size=(10, 12), seed=5)
    xa, ya = ds.batch(torch.tensor([3, 7, 1]), epoch=2)
    xb, yb = ds.batch(torch.tensor([9, 1, 0, 3, 3]), epoch=2)
    assert xa.shape == (3, 3, 10, 12) and torch.equal(ya, torch.tensor([13, 17, 11]))
    assert torch.equal(xa[0], xb[3]) and torch.equal(xa[0], xb[4]) and torch.equal(xa[2], xb[1])
    assert ds.redraws == 1
    xc, _ = ds.batch(torch.tensor([3]), epoch=3)
    assert ds.redraws == 2 and not torch.equal(xc[0], xa[0])
    # a second dataset (a resumed run) repeats the epoch
    again = DeviceImageDataset(data, labels, "cpu", rrc=RrcConfig(), out_size=(10, 12), seed=5)
    assert torch.equal(again.batch(torch.tensor([3, 7, 1]), epoch=2)[0], xa)


# ----------------------------------------------- the box rule ------------------------------------------------
def test_non_fallback_boxes_keep_the_area_and_ratio_bounds():
    H, W, cfg = 64, 80, RrcConfig(scale=(0.2, 0.6), ratio=(0.5, 2.0))
    top, left, h, w, _ = draw_rrc(cfg, 3, 1, 2000, H, W).astype(np.float64).T
    # w = round(sqrt(area r)), h = round(sqrt(area / r)): each side is within 0.5 of its real value, so the real
    # area lies between (w - .5)(h - .5) and (w + .5)(h + .5), the real ratio between (w - .5)/(h + .5) and
    # (w + .5)/(h - .5).  With these bounds nine tries in ten are valid, so no row is a fallback.
    assert ((w - 0.5) * (h - 0.5) <= 0.6 * H * W).all() and ((w + 0.5) * (h + 0.5) >= 0.2 * H * W).all()
    assert ((w - 0.5) / (h + 0.5) <= 2.0).all() and ((w + 0.5) / (h - 0.5) >= 0.5).all()
    assert len(np.unique(w)) > 10 and len(np.unique(top)) > 10 and len(np.unique(left)) > 10


def test_full_scale_square_ratio_is_the_whole_image():
    t = draw_rrc(RrcConfig(scale=(1, 1), ratio=(1, 1), hflip=0.0), 0, 0, 20, 32, 32)
    assert (t == np.array([0, 0, 32, 32, 0])).all()


def test_unsatisfiable_scale_takes_the_clamped_centred_fallback():
    # area = H W with ratio <= 4/3 on a 20 x 60 source: w <= W needs h >= 45 > H -- no try is valid
    cfg = RrcConfig(scale=(1, 1), ratio=(3 / 4, 4 / 3), hflip=0.0)
    t = draw_rrc(cfg, 0, 0, 10, 20, 60)
    assert (t == np.array([0, (60 - 27) // 2, 20, 27, 0])).all()         # h = H, w = round(H * 4/3)
    t = draw_rrc(cfg, 0, 0, 10, 60, 20)
    assert (t == np.array([(60 - 27) // 2, 0, 27, 20, 0])).all()         # w = W, h = round(W / (3/4))
    # a ratio inside the bounds leaves the whole image
    t = draw_rrc(RrcConfig(scale=(4, 4), hflip=0.0), 0, 0, 10, 30, 32)
    assert (t == np.array([0, 0, 30, 32, 0])).all()


def test_center_box_and_config_checks():
    assert center_box(40, 48, 0.875) == (2, 6, 35, 35, 0)
    assert center_box(256, 256, 0.875) == (16, 16, 224, 224, 0)
    assert center_box(5, 9, 1.0) == (0, 2, 5, 5, 0)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            center_box(8, 8, bad)
    for kw in ({"scale": (0.0, 1.0)}, {"scale": (0.5, 0.2)}, {"ratio": (1.0,)}, {"ratio": (-1, 1)}, {"hflip": 1.5}):
        with pytest.raises(ValueError):
            RrcConfig(**kw)


# ----------------------------------------------- the resampling ----------------------------------------------
def test_tap_ranges_are_those_of_the_real_valued_rule():
    for n, m in [(41, 24), (37, 7), (1, 9), (3, 24), (5, 16), (64, 7), (16, 16), (63, 7)]:
        lo, hi = rrc_taps(n, m)
        scale = n / m
        support = max(scale, 1.0)
        for i in range(m):
            c = scale * (i + 0.5)
            # away from exact ties the floating-point form gives the same integers
            a, b = c - support + 0.5, c + support + 0.5
            if abs(a - round(a)) > 1e-9:
                assert lo[i] == max(0, math.floor(a))
            if abs(b - round(b)) > 1e-9:
                assert hi[i] == min(n, math.floor(b))
        assert (hi > lo).all() and (lo >= 0).all() and (hi <= n).all()
        assert int((hi - lo).max()) <= 2 * support + 2
        wts = rrc_weights(n, m, torch.float64)
        assert torch.allclose(wts.sum(1), torch.ones(m, dtype=torch.float64), atol=1e-14) and (wts >= 0).all()


@pytest.mark.parametrize("group", sorted(R.GROUPS))
def test_reference_matches_interpolate_antialias_in_fp64(group):
    (H, W), (Ho, Wo), rows = R.GROUPS[group]
    data, labels = R.source(H, W)
    table = R.table_of(rows)
    got, lab = rrc_reference(data, labels, R.IDX, table, Ho, Wo, R.MEAN, R.STD, dtype=torch.float64)
    want = R.yardstick(data, R.IDX, table, Ho, Wo)
    err = (got - want).abs().amax(dim=(1, 2, 3))
    print(group, "fp64 reference vs F.interpolate, per sample:", err.tolist())
    assert got.dtype == torch.float64 and got.shape == (5, 3, Ho, Wo)
    assert float(err.max()) <= 1e-12
    assert torch.equal(lab, torch.as_tensor(labels)[R.IDX])
    # the fp32 path is the same rule in fp32
    got32, _ = rrc_reference(data, labels, R.IDX, table, Ho, Wo, R.MEAN, R.STD)
    assert got32.dtype == torch.float32 and float((got32.double() - want).abs().max()) < 1e-5


def test_flip_mirrors_the_columns_bit_exactly():
    (H, W), (Ho, Wo), rows = R.GROUPS["to16x24"]
    data, labels = R.source(H, W)
    for dtype in (torch.float32, torch.float64):
        out, _ = rrc_reference(data[:1].repeat(2, axis=0), labels[:2], [0, 1],
                               R.table_of([(3, 4, 30, 20, 0), (3, 4, 30, 20, 1)]), Ho, Wo, R.MEAN, R.STD, dtype=dtype)
        assert torch.equal(out[1], out[0].flip(-1)) and not torch.equal(out[1], out[0])


@pytest.mark.parametrize("C", [3, 1])
def test_identity_box_is_bit_equal_to_the_plain_batch(C):
    data, labels = R.source(37, 41, C=C)
    idx = torch.tensor(R.IDX)
    table = R.table_of([(0, 0, 37, 41, 0)] * 4)
    got, lab = rrc_reference(data, labels, idx, table, 37, 41, R.MEAN, R.STD)
    want, wlab = image_batch_reference(torch.as_tensor(data), torch.as_tensor(labels), idx, 4, False, 0, 0, R.MEAN,
                                       R.STD)
    assert torch.equal(got, want) and torch.equal(lab, wlab)
    # an identity-sized box elsewhere is that window of the plain batch
    got, _ = rrc_reference(data, labels, idx, R.table_of([(5, 9, 16, 24, 0)] * 4), 16, 24, R.MEAN, R.STD)
    assert torch.equal(got, want[:, :, 5:21, 9:33])


def test_reference_refuses_a_bad_table():
    data, labels = R.source(20, 24)
    for row, match in [((0, 0, 21, 24, 0), "inside"), ((-1, 0, 4, 4, 0), "inside"), ((0, 21, 4, 4, 0), "inside"),
                       ((0, 0, 0, 4, 0), "h or w"), ((0, 0, 4, 4, 2), "flip"), ((0, 0, 20, 24, 0), "down-scaled")]:
        with pytest.raises(ValueError, match=match):
            rrc_reference(data, labels, [0], R.table_of([row] * 4), 1, 8, R.MEAN, R.STD)
    with pytest.raises(ValueError, match="exclude"):
        DeviceImageDataset(data, labels, "cpu", rrc=RrcConfig(), eval_crop=0.9)
    with pytest.raises(ValueError, match="out_size needs"):
        DeviceImageDataset(data, labels, "cpu", out_size=8)


def test_eval_crop_dataset_and_default_dataset():
    data, labels = R.source(20, 24, N=6)
    ds = DeviceImageDataset(data, labels, "cpu", eval_crop=0.8, out_size=8, mean=R.MEAN, std=R.STD)
    idx = torch.tensor([5, 0, 2])
    x, y = ds.batch(idx, epoch=0)
    box = center_box(20, 24, 0.8)
    assert box == (2, 4, 16, 16, 0)
    want, _ = rrc_reference(data, labels, idx, R.table_of([box] * 6), 8, 8, R.MEAN, R.STD)
    assert torch.equal(x, want) and torch.equal(y, torch.tensor([15, 10, 12]))
    assert torch.equal(ds.batch(idx, epoch=9)[0], x) and ds.redraws == 1          # one table for every epoch
    out = (torch.zeros(3, 3, 8, 8), torch.zeros(3, dtype=torch.int64))
    assert ds.batch(idx, out=out)[0] is out[0] and torch.equal(out[0], x)
    # with none of the new arguments the class is the crop/flip pipeline of the stored size
    plain = DeviceImageDataset(data, labels, "cpu", augment=True, seed=3)
    assert not plain.resample
    want, _ = image_batch_reference(plain.data, plain.labels, idx, 4, True, 3, 1, plain.mean, plain.std)
    assert torch.equal(plain.batch(idx, epoch=1)[0], want)


# ----------------------------------------------- the trainer -------------------------------------------------
def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "pytorch/resnet/main.py", *args], cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=timeout)


def _losses(out):
    return dict(re.findall(r"Epoch: (\d+), Loss: (\S+)", out))


def test_trainer_on_npy_arrays_and_exact_resume(tmp_path):
    R.write_arrays(tmp_path / "data")
    base = ["--device", "cpu", "--backend", "gloo", "--workers", "0", "--data_format", "npy", "--data_root",
            str(tmp_path / "data"), "--image_size", "32", "--num_classes", "4", "--batch_size", "16", "--eval_every", "1"]
    r = _run(base + ["--num_epochs", "2", "--model_dir", str(tmp_path / "a")])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    whole = _losses(r.stdout)
    assert set(whole) == {"0", "1"} and all(math.isfinite(float(v)) for v in whole.values())
    assert r.stdout.count("Accuracy") == 2
    r = _run(base + ["--num_epochs", "1", "--model_dir", str(tmp_path / "b")])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert _losses(r.stdout) == {"0": whole["0"]}
    r = _run(base + ["--num_epochs", "2", "--model_dir", str(tmp_path / "b"), "--resume"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert _losses(r.stdout) == {"1": whole["1"]}                     # the resumed run repeats epoch 1


def test_npy_refuses_the_host_pipeline_and_bad_crops():
    from deeplearning_mpi_amd.apps import classification as cls

    for bad, flag in ([["--data_on_device", "0"], "--data_on_device 0"], [["--eval_crop", "0"], "--eval_crop"],
                      [["--rrc_scale", "0.5", "0.1"], "--rrc_scale"], [["--rrc_ratio", "0", "1"], "--rrc_scale"]):
        r = _run(["--device", "cpu", "--backend", "gloo", "--data_format", "npy", *bad], timeout=120)
        assert r.returncode == 2 and "error: " in r.stderr and flag in r.stderr, r.stderr[-2000:]
    # without npy the same flags are not looked at
    p = cls.build_argparser()
    cls.check_data_args(p, p.parse_args(["--data_on_device", "0"]))


def test_default_flags_build_the_loaders_of_before(monkeypatch):
    from torch.utils.data import DataLoader

    from deeplearning_mpi_amd.apps import classification as cls
    from deeplearning_mpi_amd.data import CIFAR10, DeviceBatches
    from deeplearning_mpi_amd.data.datasets import CIFAR_MEAN, CIFAR_STD

    g = np.random.default_rng(1)
    monkeypatch.setattr(CIFAR10, "_load", staticmethod(
        lambda root, train: (g.integers(0, 256, (24, 32, 32, 3), dtype=np.uint8), list(range(24)))))
    args = cls.build_argparser().parse_args(["--batch_size", "8", "--workers", "0"])
    assert (args.data_format, args.rrc_scale, args.rrc_ratio, args.eval_crop, args.norm) == \
        ("cifar10", [0.08, 1.0], [0.75, 1.3333], 0.875, None)
    assert cls.input_side(args) == 32 and cls.norm_of(args) == (CIFAR_MEAN, CIFAR_STD)
    args.graph = False
    dev = torch.device("cpu")
    train_set, sampler, train_loader, test_loader = cls.build_loaders(args, dev, None, None)   # the host pipeline
    assert isinstance(train_set, CIFAR10) and isinstance(train_loader, DataLoader)
    assert isinstance(test_loader, DataLoader) and train_loader.sampler is sampler
    assert torch.equal(train_set.transform.mean.flatten(), torch.tensor(CIFAR_MEAN))
    args.data_on_device = "1"
    train_set, sampler, train_loader, test_loader = cls.build_loaders(args, dev, None, None)
    for ds, augment in ((train_set, True), (test_loader.ds, False)):
        assert isinstance(ds, DeviceImageDataset) and not ds.resample and ds.rrc is None and ds.eval_crop is None
        assert (ds.augment, ds.pad, ds.mix, (ds.H, ds.W)) == (augment, 4, None, (32, 32))
        assert ds.mean == list(CIFAR_MEAN) and ds.std == list(CIFAR_STD)
    assert isinstance(train_loader, DeviceBatches) and train_loader.out is None
    x, y = next(iter(train_loader))
    assert x.shape == (8, 3, 32, 32)
    # npy: --image_size is the side of the step's inputs, and the constants follow the format
    args = cls.build_argparser().parse_args(["--data_format", "npy", "--image_size", "24"])
    assert cls.input_side(args) == 24 and cls.norm_of(args)[0] == (0.485, 0.456, 0.406)
    assert cls.rrc_config(args) == RrcConfig(scale=(0.08, 1.0), ratio=(0.75, 1.3333))


# ----------------------------------------------- the converter -----------------------------------------------
def test_converter_writes_the_two_arrays(tmp_path):
    from PIL import Image

    g = np.random.default_rng(2)
    sizes = {"cat": [(50, 30), (20, 20)], "dog": [(31, 64), (40, 41), (12, 90)]}      # (width, height)
    for name, dims in sizes.items():
        os.makedirs(tmp_path / "src" / name)
        for k, (w, h) in enumerate(dims):
            Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / "src" / name / f"{k}.png")
    Image.fromarray(g.integers(0, 256, (9, 9), dtype=np.uint8)).save(tmp_path / "src" / "cat" / "grey.png")   # mode L
    (tmp_path / "src" / "cat" / "notes.txt").write_text("not an image")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_image_arrays.py"), str(tmp_path / "src"),
                        str(tmp_path / "out"), "--split", "val", "--size", "24"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    images = np.load(tmp_path / "out" / "val_images.npy")
    labels = np.load(tmp_path / "out" / "val_labels.npy")
    assert images.dtype == np.uint8 and images.shape == (6, 24, 24, 3)
    assert labels.dtype == np.int64 and labels.tolist() == [0, 0, 0, 1, 1, 1]
    assert (tmp_path / "out" / "val_classes.txt").read_text().split() == ["cat", "dog"]
    assert images.std() > 20 and (images[2, ..., 0] == images[2, ..., 2]).all()       # the grey image, as RGB
    # the loader takes what the converter wrote
    ds = DeviceImageDataset.from_npy(str(tmp_path / "out"), "val", "cpu", eval_crop=0.875, out_size=16)
    x, y = ds.batch(torch.tensor([5, 0]))
    assert x.shape == (2, 3, 16, 16) and y.tolist() == [1, 0]
