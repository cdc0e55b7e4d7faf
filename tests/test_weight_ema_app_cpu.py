"""The trainers with --ema_decay on CPU / gloo: the averaged checkpoint in the reference's layout, the EMA accuracy
/ Dice lines and history, exact resume of the average, and the defaults that build none of it."""
import os

import pytest
import torch

from deeplearning_mpi_amd.models import resnet18
from deeplearning_mpi_amd.utils.checkpoint import load_checkpoint

CLS = ["--synthetic", "--device", "cpu", "--backend", "gloo", "--workers", "0", "--batch_size", "4", "--synthetic_size",
       "12", "--eval_every", "1"]
SEG = ["--device", "cpu", "--backend", "gloo", "--synthetic", "--synthetic_size", "4", "--image_size", "32",
       "--batch_size", "2", "--workers", "0", "--eval_every", "1"]
EMA = ["--ema_decay", "0.9"]


def _cls(model_dir, epochs, extra=()):
    from deeplearning_mpi_amd.apps import classification as app

    return app.main("main", [*CLS, "--num_epochs", str(epochs), "--model_dir", str(model_dir), *extra])


def _tensors(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_tensors(v, f"{prefix}{k}."))
        elif isinstance(v, torch.Tensor):
            out[prefix + k] = v
    return out


@pytest.fixture(scope="module")
def two_epochs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ema_a")
    return d, _cls(d, 2, EMA)


def test_ema_checkpoint_and_history(two_epochs, capsys):
    d, history = two_epochs
    main, avg = d / "resnet_distributed.pth", d / "resnet_distributed.ema.pth"
    assert avg.exists() and not os.path.exists(str(avg) + ".state")
    w, e = torch.load(main, weights_only=True), torch.load(avg, weights_only=True)
    assert list(w) == list(e) and all(k.startswith("module.") for k in e)       # the reference's layout
    assert all(w[k].shape == e[k].shape and w[k].dtype == e[k].dtype for k in w)
    assert any(not torch.equal(w[k], e[k]) for k in w if "num_batches" not in k)
    assert all(torch.equal(w[k], e[k]) for k in w if "num_batches" in k)
    fresh = resnet18(num_classes=10)
    load_checkpoint(fresh, str(avg), map_location="cpu")
    assert all(torch.equal(v, e["module." + k]) for k, v in fresh.state_dict().items())
    assert len(history["ema_accuracy"]) == len(history["accuracy"]) == 2
    assert all(0.0 <= a <= 1.0 for a in history["ema_accuracy"])
    # the sidecar's average is the checkpoint's
    sd = torch.load(str(main) + ".state", weights_only=True)["ema"]
    assert all(torch.equal(v, e["module." + k]) for k, v in {**sd["params"], **sd["buffers"]}.items())
    assert sd["state"].tolist()[:2] == [6, 6] and (sd["decay"], sd["warmup"], sd["every"]) == (0.9, True, 1)


def test_ema_accuracy_line(tmp_path, capsys):
    _cls(tmp_path, 1, [*EMA, "--ema_every", "2", "--ema_warmup", "0"])
    out = capsys.readouterr().out
    assert "Epoch: 0, Accuracy: " in out and "Epoch: 0, EMA Accuracy: " in out
    sd = torch.load(str(tmp_path / "resnet_distributed.pth") + ".state", weights_only=True)["ema"]
    assert sd["state"].tolist()[:2] == [3, 1] and (sd["warmup"], sd["every"]) == (False, 2)


def test_resume_reproduces_the_average_bit_for_bit(two_epochs, tmp_path):
    a, _ = two_epochs
    _cls(tmp_path, 1, EMA)
    _cls(tmp_path, 2, [*EMA, "--resume"])
    for name in ("resnet_distributed.pth", "resnet_distributed.ema.pth"):
        wa, wb = torch.load(a / name, weights_only=True), torch.load(tmp_path / name, weights_only=True)
        assert wa.keys() == wb.keys() and all(torch.equal(wa[k], wb[k]) for k in wa), name
    sa = _tensors(torch.load(str(a / "resnet_distributed.pth") + ".state", weights_only=True)["ema"])
    sb = _tensors(torch.load(str(tmp_path / "resnet_distributed.pth") + ".state", weights_only=True)["ema"])
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_defaults_build_nothing(tmp_path):
    history = _cls(tmp_path, 1)
    assert "ema_accuracy" not in history
    assert sorted(os.listdir(tmp_path)) == ["resnet_distributed.pth", "resnet_distributed.pth.state"]
    assert "ema" not in torch.load(str(tmp_path / "resnet_distributed.pth") + ".state", weights_only=True)


@pytest.mark.parametrize("bad", [["--ema_decay", "1.0"], ["--ema_decay", "-0.5"], ["--ema_decay", "nan"],
                                 ["--ema_decay", "0.9", "--ema_every", "0"]])
def test_invalid_flags_are_argparse_errors(bad, capsys):
    from deeplearning_mpi_amd.apps import classification as cls, segmentation as seg

    with pytest.raises(SystemExit) as e:
        cls.main("main", [*CLS, *bad])
    assert e.value.code == 2 and "--ema_" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        seg.parse_args([*SEG, *bad])
    assert e.value.code == 2 and "--ema_" in capsys.readouterr().err


@pytest.mark.parametrize("optimizer", ["adam", "lamb"])
def test_unet_trainer_with_ema(tmp_path, capsys, optimizer):
    from deeplearning_mpi_amd.apps import segmentation as seg

    args = seg.parse_args([*SEG, "--num_epochs", "1", "--log_dir", str(tmp_path / "logs"), "--model_dir", str(tmp_path),
                           "--optimizer", optimizer, *EMA])
    history = seg.run(args)
    out = capsys.readouterr().out
    assert "Epoch 1 Dice Score: " in out and "Epoch 1 EMA Dice Score: " in out and "FINAL DICE COEFFICIENT" in out
    assert len(history["ema_dice"]) == len(history["dice"]) == 1 and "final_ema_dice" in history
    w = torch.load(tmp_path / "model.pth", weights_only=True)
    e = torch.load(tmp_path / "model.ema.pth", weights_only=True)
    assert list(w) == list(e) and any(not torch.equal(w[k], e[k]) for k in w)
    sd = torch.load(str(tmp_path / "model.pth") + ".state", weights_only=True)["ema"]
    assert sd["state"].tolist()[:3] == [2, 2, 2]          # both updates applied, the optimizer's counter seen

    args = seg.parse_args([*SEG, "--num_epochs", "1", "--log_dir", str(tmp_path / "logs"),
                           "--model_dir", str(tmp_path / "plain"), "--optimizer", optimizer])
    history = seg.run(args)
    assert "ema_dice" not in history and "final_ema_dice" not in history
    assert sorted(os.listdir(tmp_path / "plain")) == ["model.pth", "model.pth.state", "model.pth.state.prev"]
    assert "ema" not in torch.load(str(tmp_path / "plain" / "model.pth") + ".state", weights_only=True)
