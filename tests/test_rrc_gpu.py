"""The RandomResizedCrop batch kernel (csrc/kernels/rrc.hip) against rrc_reference (itself tied to torch's
F.interpolate(antialias=True) in tests/test_rrc_cpu.py), its bit-exact cases, its determinism, the binding's
refusals and the classification trainer on .npy arrays with and without the captured step.

Tolerance of the kernel, per sample of every case: the yardstick is the fp64 F.interpolate result; the fp32 CPU
rrc_reference has some error against it, computed here (9e-8 to 5.6e-6 after the division by a std of 0.2: the
largest where scale = n / m is no binary fraction and the fp32 centres carry its rounding), and the kernel -- the
same rule with another summation order and FMA contraction -- is allowed 4x that error.  Measured on an MI355X:
at most 1.63x (profiles/rrc/README.md)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import rrc_cases as R
import torch

from deeplearning_mpi_amd.data import DeviceImageDataset, RrcConfig, draw_rrc, rrc_reference
from deeplearning_mpi_amd.data.rrc import MAX_SCALE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _native():
    from deeplearning_mpi_amd._ext import native

    return native()


def _gpu(data, labels, idx, table):
    return (torch.as_tensor(data).to(DEV), torch.as_tensor(labels).to(DEV),
            torch.as_tensor(idx, dtype=torch.int64).to(DEV), torch.as_tensor(table).to(DEV))


def _launch(data, labels, idx, table, Ho, Wo, out=None):
    d, l, i, t = _gpu(data, labels, idx, table)
    C = d.shape[-1]
    x = torch.empty(len(idx), C, Ho, Wo, device=DEV) if out is None else out
    y = torch.full((len(idx),), -1, dtype=torch.int64, device=DEV)
    _native().image_rrc_batch(d, l, i, t, list(R.MEAN[:C]), list(R.STD[:C]), x, y)
    return x, y


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("group", sorted(R.GROUPS))
def test_kernel_within_four_times_the_fp32_reference_error(group, C):
    (H, W), (Ho, Wo), rows = R.GROUPS[group]
    data, labels = R.source(H, W, C=C)
    table = R.table_of(rows)
    yard = R.yardstick(data, R.IDX, table, Ho, Wo)
    ref32, _ = rrc_reference(data, labels, R.IDX, table, Ho, Wo, R.MEAN, R.STD)
    ref_err = (ref32.double() - yard).abs().amax(dim=(1, 2, 3))
    outs = {"packed": _launch(data, labels, R.IDX, table, Ho, Wo)}
    # the same batch into a view that starts 4 bytes into its storage: the scalar store path whatever Wo is
    store = torch.zeros(5 * C * Ho * Wo + 1, device=DEV)
    outs["offset"] = _launch(data, labels, R.IDX, table, Ho, Wo, out=store[1:].view(5, C, Ho, Wo))
    assert outs["offset"][0].data_ptr() % 16 == 4
    for name, (x, y) in outs.items():
        err = (x.cpu().double() - yard).abs().amax(dim=(1, 2, 3))
        print(f"{group} C={C} {name}: kernel error {[f'{e:.3g}' for e in err.tolist()]} "
              f"fp32 reference error {[f'{e:.3g}' for e in ref_err.tolist()]}")
        assert (err <= 4 * ref_err).all(), (name, err.tolist(), ref_err.tolist())
        assert torch.equal(y.cpu(), torch.as_tensor(labels)[R.IDX])
    assert float(store[0]) == 0.0
    # the two store paths run the same arithmetic
    assert torch.equal(outs["packed"][0], outs["offset"][0])


@pytest.mark.parametrize("H,W,C", [(37, 41, 3), (12, 16, 3), (12, 16, 1)])
def test_identity_and_flip_are_bit_equal_to_the_plain_batch(H, W, C):
    data, labels = R.source(H, W, C=C)
    d, l, i, _ = _gpu(data, labels, R.IDX, R.table_of([(0, 0, H, W, 0)] * 4))
    plain = torch.empty(5, C, H, W, device=DEV)
    py = torch.empty(5, dtype=torch.int64, device=DEV)
    _native().image_batch(d, l, i, H, W, C, 4, False, 0, 0, list(R.MEAN[:C]), list(R.STD[:C]), plain, py)
    x, y = _launch(data, labels, R.IDX, R.table_of([(0, 0, H, W, 0)] * 4), H, W)
    assert torch.equal(x, plain) and torch.equal(y, py)
    x, _ = _launch(data, labels, R.IDX, R.table_of([(0, 0, H, W, 1)] * 4), H, W)
    assert torch.equal(x, plain.flip(-1)) and not torch.equal(x, plain)
    # an identity-sized box elsewhere is that window
    x, _ = _launch(data, labels, R.IDX, R.table_of([(3, 5, 8, 8, 0)] * 4), 8, 8)
    assert torch.equal(x, plain[:, :, 3:11, 5:13])


def test_determinism_out_and_batch_composition():
    data, labels = R.source(40, 48, N=12)
    ds = DeviceImageDataset(data, labels, DEV, rrc=RrcConfig(), out_size=(20, 28), seed=5, mean=R.MEAN, std=R.STD)
    ia, ib = torch.tensor([3, 7, 1], device=DEV), torch.tensor([9, 1, 0, 3, 3], device=DEV)
    xa, ya = ds.batch(ia, epoch=2)
    xa2, _ = ds.batch(ia, epoch=2)
    assert xa.shape == (3, 3, 20, 28) and torch.equal(xa, xa2) and ya.tolist() == [13, 17, 11]
    out = (torch.zeros(3, 3, 20, 28, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV))
    got = ds.batch(ia, epoch=2, out=out)
    assert got[0] is out[0] and torch.equal(out[0], xa) and torch.equal(out[1], ya)
    xb, _ = ds.batch(ib, epoch=2)
    assert torch.equal(xa[0], xb[3]) and torch.equal(xa[0], xb[4]) and torch.equal(xa[2], xb[1])
    assert ds.redraws == 1
    # the device batch is the reference's, through the drawn table
    table = draw_rrc(RrcConfig(), 5, 2, 12, 40, 48)
    ref, _ = rrc_reference(data, labels, ib.cpu(), table, 20, 28, R.MEAN, R.STD)
    assert float((xb.cpu() - ref).abs().max()) < 1e-5
    xc, _ = ds.batch(ia, epoch=3)
    assert ds.redraws == 2 and not torch.equal(xc, xa)
    with pytest.raises(ValueError, match="out must be"):
        ds.batch(ia, epoch=3, out=(torch.zeros(3, 3, 20, 24, device=DEV), out[1]))
    # evaluation: the centre box, one table for every epoch
    ev = DeviceImageDataset(data, labels, DEV, eval_crop=0.875, out_size=20, mean=R.MEAN, std=R.STD)
    xe, _ = ev.batch(ia, epoch=0)
    ref, _ = rrc_reference(data, labels, ia.cpu(), R.table_of([(2, 6, 35, 35, 0)] * 12), 20, 20, R.MEAN, R.STD)
    assert float((xe.cpu() - ref).abs().max()) < 1e-5 and torch.equal(ev.batch(ia, epoch=4)[0], xe)


def test_binding_refuses_bad_arguments_before_any_launch():
    f = _native().image_rrc_batch
    data, labels = R.source(20, 24)
    good = R.table_of([(0, 0, 20, 24, 0), (1, 2, 3, 4, 1), (5, 5, 15, 19, 0), (19, 23, 1, 1, 1)])
    d, l, i, t = _gpu(data, labels, R.IDX, good)
    mean, std = list(R.MEAN), list(R.STD)
    x = torch.full((5, 3, 8, 12), 7.0, device=DEV)
    y = torch.full((5,), -1, dtype=torch.int64, device=DEV)
    f(d, l, i, t, mean, std, x, y)                                   # the arguments below differ in one thing each
    assert y.tolist() == [13, 12, 12, 10, 11] and not (x == 7.0).any()

    def tab(row, at=2):
        rows = good.copy()
        rows[at] = row
        return torch.as_tensor(rows).to(DEV)

    cap = _native().rrc_max_scale()
    assert cap == MAX_SCALE == 15            # the CPU path checks its tables against the same cap
    x.fill_(7.0)
    y.fill_(-1)
    small = torch.full((5, 3, 1, 12), 7.0, device=DEV)
    d2 = d[..., :2].contiguous()
    bad = [
        ("row below the image", dict(table=tab((6, 0, 15, 24, 0))), "table row 2 .*does not lie inside the 20 x 24"),
        ("row right of the image", dict(table=tab((0, 21, 4, 4, 0), at=3)), "table row 3 .*does not lie inside"),
        ("negative corner", dict(table=tab((-1, 0, 4, 4, 0))), "does not lie inside"),
        ("h = 0", dict(table=tab((3, 3, 0, 4, 0))), "h and w must be at least 1"),
        ("w = 0", dict(table=tab((3, 3, 4, 0, 1))), "h and w must be at least 1"),
        ("flip = 2", dict(table=tab((3, 3, 4, 4, 2))), "flip must be 0 or 1"),
        ("box past the tap cap", dict(x=small), f"down-scaled by more than {cap}x"),
        ("float table", dict(table=t.float()), "int32 table"),
        ("int32 indices", dict(idx=i.int()), "int64 labels and indices"),
        ("float data", dict(data=d.float()), "uint8 data"),
        ("fp64 output", dict(x=x.double()), "fp32 output"),
        ("int32 output labels", dict(y=y.int()), "int64 output labels"),
        ("non-contiguous output", dict(x=torch.full((5, 3, 12, 8), 7.0, device=DEV).transpose(2, 3)), "contiguous"),
        ("non-contiguous table", dict(table=torch.as_tensor(np.ascontiguousarray(good.T)).to(DEV).t()), "contiguous"),
        ("C = 2", dict(data=d2, mean=mean[:2], std=std[:2], x=torch.full((5, 2, 8, 12), 7.0, device=DEV)),
         "C must be 1 or 3"),
        ("table of another length", dict(table=t[:3].contiguous()), r"table must be \[N, 5\]"),
        ("table of 6 columns", dict(table=torch.zeros(4, 6, dtype=torch.int32, device=DEV)), r"table must be \[N, 5\]"),
        ("output of another batch", dict(x=torch.full((4, 3, 8, 12), 7.0, device=DEV)), r"out must be \[B, C, Ho, Wo\]"),
        ("output labels of another batch", dict(y=y[:4].contiguous()), r"out_labels must be \[B\]"),
        ("mean of two", dict(mean=mean[:2]), "mean/std per channel"),
        ("host table", dict(table=t.cpu()), "on the GPU"),
        ("host output", dict(x=x.cpu()), "on the GPU"),
    ]
    for name, change, match in bad:
        a = dict(data=d, labels=l, idx=i, table=t, mean=mean, std=std, x=x, y=y)
        a.update(change)
        x.fill_(7.0)
        y.fill_(-1)
        with pytest.raises(RuntimeError, match="image_rrc_batch: .*" + match):
            f(a["data"], a["labels"], a["idx"], a["table"], a["mean"], a["std"], a["x"], a["y"])
        torch.cuda.synchronize()
        assert (a["x"] == 7.0).all() and (y == -1).all(), name         # nothing was launched
    # a table changed in place is checked again
    t2 = t.clone()
    f(d, l, i, t2, mean, std, x, y)
    t2[1, 2] = 25
    with pytest.raises(RuntimeError, match="table row 1 .*does not lie inside"):
        f(d, l, i, t2, mean, std, x, y)


def _run(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "pytorch/resnet/main.py", *args], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_trainer_graph_matches_eager_and_mixup_runs(tmp_path):
    R.write_arrays(tmp_path / "data")
    base = ["--data_format", "npy", "--data_root", str(tmp_path / "data"), "--image_size", "32", "--num_classes", "4",
            "--batch_size", "16", "--num_epochs", "1", "--steps_per_epoch", "3", "--workers", "0"]
    out_e = _run(base + ["--model_dir", str(tmp_path / "e"), "--graph", "0"])
    out_g = _run(base + ["--model_dir", str(tmp_path / "g"), "--graph", "1"])
    assert "capture failed" not in out_g
    loss = [re.findall(r"Epoch: \d+, Loss: (\S+)", o) for o in (out_e, out_g)]
    assert len(loss[0]) == 1 and loss[0] == loss[1] and np.isfinite(float(loss[0][0]))
    assert "(3 steps)" in out_e and "(3 steps)" in out_g and "Accuracy" in out_g
    out_m = _run(base + ["--model_dir", str(tmp_path / "m"), "--graph", "1", "--mixup_alpha", "0.2"])
    mixed = re.findall(r"Epoch: \d+, Loss: (\S+)", out_m)
    assert len(mixed) == 1 and np.isfinite(float(mixed[0])) and mixed != loss[0] and "capture failed" not in out_m
