"""ops.surface_distances on the CPU path (RefBackend) against the brute-force reference of tests/surface_ref.py, its
argument checks, and the trainer's --eval_surface line.  Tolerances (derived in surface_ref.check): counts and the
Hausdorff column exact, the percentile and ASSD columns within one fp32 ulp of the rounded fp64 reference."""
import glob

import pytest
import torch

import surface_ref as R
from deeplearning_mpi_amd.ops import surface_distances


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_matches_brute_force(case):
    x, t = R.device_inputs(case, "cpu")
    R.check(*surface_distances(x, t, R.IGNORE, case[5]), case)


def test_layouts_agree_and_bad_arguments_raise():
    case = R.CASES[0]
    a = surface_distances(*R.device_inputs(case, "cpu"), R.IGNORE)
    x, t = R.device_inputs(case, "cpu", "nhwc_view")
    b = surface_distances(x, t, R.IGNORE)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for bad in (0.0, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            surface_distances(x, t, percentile=bad)
    with pytest.raises(ValueError):
        surface_distances(x, t.float())            # K logits with a float target
    with pytest.raises(ValueError):
        surface_distances(x[:, 0], t[:, :-1].float())   # shapes differ
    with pytest.raises(ValueError):
        surface_distances(x, t[:, :-1])


SEG = ["--device", "cpu", "--backend", "gloo", "--synthetic", "--synthetic_size", "4", "--image_size", "32",
       "--batch_size", "2", "--workers", "0", "--eval_every", "1", "--num_epochs", "1"]


def test_trainer_reports_surface_distances(tmp_path, classes="3"):
    from deeplearning_mpi_amd.apps import segmentation as seg

    def train(name, extra):
        logs = tmp_path / name
        h = seg.run(seg.parse_args(SEG + ["--num_classes", classes, "--log_dir", str(logs), "--model_dir",
                                          str(tmp_path / (name + "_m"))] + extra))
        (log,) = glob.glob(str(logs / "training_log_*.log"))
        lines = [ln for ln in open(log).read().splitlines() if ln.startswith("Epoch 1 |")]
        return h, [ln.split(" | ")[1].split(":")[0] for ln in lines]

    h0, lines0 = train("off", [])
    h1, lines1 = train("on", ["--eval_surface", "1", "--ema_decay", "0.9"])
    assert lines0 == ["Loss", "Dice Score"] and "hd95" not in h0 and "assd" not in h0
    assert lines1 == ["Loss", "Dice Score", "HD95", "EMA Dice Score", "EMA HD95"]
    assert len(h1["hd95"]) == len(h1["assd"]) == len(h1["ema_hd95"]) == 1 and "final_hd95" in h1
    assert h1["dice"] == h0["dice"] and h1["loss"] == h0["loss"]
