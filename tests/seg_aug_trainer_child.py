"""Child process of tests/test_seg_aug_gpu.py: the UNet trainer with the --aug_* flags on the GPU, once eagerly
and once with the captured step, for each synthetic set size given on the command line.  Prints one JSON line
per run: the loss history, how many parameter tables the training set drew, how many batches it served, how
often the captured step replayed and whether the batch kernel wrote the captured step's inputs in place."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deeplearning_mpi_amd.apps import segmentation as seg  # noqa: E402
from deeplearning_mpi_amd.data import DeviceSegDataset  # noqa: E402
from deeplearning_mpi_amd.utils import graphs  # noqa: E402

AUG = ["--aug_hflip", "0.5", "--aug_vflip", "0.5", "--aug_scale", "0.8", "1.25", "--aug_rotate", "20",
       "--aug_translate", "0.1"]


def main():
    with tempfile.TemporaryDirectory() as tmp:
        run(tmp)


def run(tmp):
    for size in sys.argv[1:]:
        for graph in ("0", "1"):
            seen = {}
            real_build, real_batch = seg.build_data_loaders, DeviceSegDataset.batch

            def build(args, device):
                seen["loaders"] = real_build(args, device)
                return seen["loaders"]

            def batch(self, idx, epoch=0, out=None):
                seen["batches"] = seen.get("batches", 0) + 1
                seen["in_place"] = seen.get("in_place", 0) + (out is not None)
                return real_batch(self, idx, epoch, out)

            seg.build_data_loaders, DeviceSegDataset.batch = build, batch
            replays = graphs.REPLAYS
            try:
                args = seg.parse_args(["--synthetic", "--synthetic_size", size, "--image_size", "32", "--batch_size",
                                       "4", "--num_epochs", "2", "--num_classes", "3", "--workers", "0",
                                       "--eval_every", "100", "--graph", graph, "--log_dir", os.path.join(tmp, "logs"),
                                       "--model_dir", tmp] + AUG)
                hist = seg.run(args)
            finally:
                seg.build_data_loaders, DeviceSegDataset.batch = real_build, real_batch
            ds = seen["loaders"][0].ds
            print(json.dumps({"size": int(size), "graph": int(graph), "loss": hist["loss"], "redraws": ds.redraws,
                              "dataset": type(ds).__name__, "device": ds.images.device.type,
                              "batches": seen["batches"], "in_place": seen["in_place"],
                              "replays": graphs.REPLAYS - replays}), flush=True)


if __name__ == "__main__":
    main()
