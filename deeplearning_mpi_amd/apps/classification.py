"""ResNet data-parallel classification training (the reference's pytorch/resnet/{main,resnet}.py).

Flags keep the reference names and defaults: --num_epochs, --batch_size (per
process), --learning_rate, --random_seed, --model_dir, --model_filename, --resume.  Non-breaking
additions: --arch, --num_classes, --synthetic, --data_root, --image_size, --backend, --device,
--bucket_mb, --workers, --eval_every, --steps_per_epoch, --precision, --graph, --data_on_device,
--benchmark_steps, --label_smoothing, --mixup_alpha, --cutmix_alpha, --mix_prob, --mix_switch_prob,
--data_format, --rrc_scale, --rrc_ratio, --eval_crop, --norm, --ema_decay, --ema_every, --ema_warmup.

--data_format npy trains on a folder's images at any size: {data_root}/train_images.npy (uint8 [N, H, W, C]) and
train_labels.npy (int64 [N]), val_* likewise (scripts/make_image_arrays.py writes them), live in device memory and
one kernel per batch does gather + RandomResizedCrop(--image_size) + flip + normalize (data/rrc.py); evaluation
is resize + centre crop (--eval_crop).

Deliberate fixes of reference quirks: the sampler's epoch is advanced every epoch;
evaluation runs on the unwrapped module (no stray rank-0-only collective, K8) with a non-augmenting
test transform; checkpoints are written by GLOBAL rank 0 only; the per-step loss stays on the
device (one host sync per epoch instead of one per step).
"""
from __future__ import annotations

import argparse
import math
import os
import random
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import parallel
from ..data import (CIFAR10, CifarTransform, DeviceBatches, DeviceImageDataset, DistributedSampler, MixConfig,
                    RrcConfig, SyntheticImages, draw_mix, mix_batch_)
from ..data.datasets import CIFAR_MEAN, CIFAR_STD, IMAGENET_MEAN, IMAGENET_STD
from ..models import ARCHS
from ..ops import CrossEntropyLoss, backward, top1_correct
from ..optim import LARS, SGD, WeightEMA
from ..utils.checkpoint import load_checkpoint, resume_state, save_checkpoint, set_rng_state
from ..utils.graphs import CapturedStep


def build_argparser(variant: str = "main") -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--num_epochs", type=int, help="Number of training epochs.", default=100)
    p.add_argument("--batch_size", type=int, help="Training batch size for one process.",
                   default=128 if variant == "main" else 32)
    p.add_argument("--learning_rate", type=float, help="Learning rate.", default=0.1)
    p.add_argument("--random_seed", type=int, help="Random seed.", default=0)
    p.add_argument("--model_dir", type=str, help="Directory for saving models.", default="saved_models")
    p.add_argument("--model_filename", type=str, help="Model filename.", default="resnet_distributed.pth")
    p.add_argument("--resume", action="store_true", help="Resume training from saved checkpoint.")
    # additions
    p.add_argument("--arch", default="resnet18", choices=sorted(ARCHS))
    p.add_argument("--num_classes", type=int, default=10)
    p.add_argument("--synthetic", action="store_true", help="random data instead of CIFAR-10")
    p.add_argument("--synthetic_size", type=int, default=1024, help="images per epoch (synthetic)")
    p.add_argument("--data_root", default="./data")
    p.add_argument("--image_size", type=int, default=32)
    p.add_argument("--backend", default="nccl", help="nccl|rccl (GPU, RCCL) or gloo (CPU)")
    p.add_argument("--device", default="auto", help="auto | cpu | cuda")
    p.add_argument("--bucket_mb", type=float, default=None)
    p.add_argument("--workers", type=int, default=8 if variant != "main" else 15)
    p.add_argument("--eval_every", type=int, default=10)
    p.add_argument("--test_batch_size", type=int, default=None if variant == "main" else 128)
    p.add_argument("--steps_per_epoch", type=int, default=0, help="cap steps per epoch (0 = full epoch)")
    p.add_argument("--eval_before_train", action="store_true", default=variant != "main",
                   help="resnet.py variant: evaluate/save before training on eval epochs")
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32"],
                   help="bf16: native gfx950 kernels on bf16 activations; fp32: the same kernels on fp32 "
                        "activations and weights (fp32 MFMA)")
    p.add_argument("--graph", nargs="?", const="1", default="auto", choices=["auto", "0", "1"],
                   help="replay each full-size training step from a captured hipGraph (ragged last batches run "
                        "eagerly); auto = on for launch-bound GPU training")
    p.add_argument("--data_on_device", default="auto", choices=["auto", "0", "1"],
                   help="keep CIFAR-10 resident in GPU memory and build each augmented batch with one kernel "
                        "(data/device.py); auto = on for GPU training on real data")
    p.add_argument("--benchmark_steps", type=int, default=0,
                   help="time this many steps on a synthetic device batch, print images/sec and exit")
    add_layerwise_args(p, "sgd", "lars")
    add_recipe_args(p)
    add_data_args(p)
    add_ema_args(p)
    return p


def add_ema_args(p):
    """Weight EMA (optim.WeightEMA): averaged weights for evaluation and a second checkpoint."""
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="decay of the exponential moving average of the weights and BatchNorm statistics, in [0, 1) "
                        "(0 = off): evaluated and checkpointed next to the trained weights")
    p.add_argument("--ema_every", type=int, default=1, help="average on every K-th applied optimizer update")
    p.add_argument("--ema_warmup", type=int, default=1, choices=[0, 1],
                   help="1: decay min(--ema_decay, (1 + s) / (10 + s)) at the s-th averaging update")


def check_ema_args(parser, args):
    if not (math.isfinite(args.ema_decay) and 0 <= args.ema_decay < 1):
        parser.error("--ema_decay must lie in [0, 1)")
    if args.ema_every < 1:
        parser.error("--ema_every must be at least 1")


def ema_of(args, model, optimizer):
    """The WeightEMA of the run, or None with --ema_decay 0 (then nothing of it is built)."""
    if not getattr(args, "ema_decay", 0.0) > 0:
        return None
    return WeightEMA(model, decay=args.ema_decay, warmup=bool(args.ema_warmup), every=args.ema_every,
                     optimizer=optimizer)


def ema_path(path: str) -> str:
    """<stem>.ema<ext>: the averaged weights next to the trained ones."""
    stem, ext = os.path.splitext(path)
    return stem + ".ema" + ext


def add_data_args(p):
    """Real images of any stored size, resampled to --image_size on the device (data/rrc.py)."""
    p.add_argument("--data_format", default="cifar10", choices=["cifar10", "npy"],
                   help="npy: {data_root}/{train,val}_images.npy + _labels.npy, kept in device memory and cropped / "
                        "resized to --image_size by the batch kernel")
    p.add_argument("--rrc_scale", type=float, nargs=2, default=[0.08, 1.0], metavar=("LO", "HI"),
                   help="npy: area of the random crop as a fraction of the stored image")
    p.add_argument("--rrc_ratio", type=float, nargs=2, default=[0.75, 1.3333], metavar=("LO", "HI"),
                   help="npy: aspect ratio (w / h) of the random crop")
    p.add_argument("--eval_crop", type=float, default=0.875,
                   help="npy: evaluation resizes the centred square of this fraction of the shorter side")
    p.add_argument("--norm", default=None, choices=["cifar", "imagenet"],
                   help="normalisation constants (default: cifar for cifar10, imagenet for npy)")


def check_data_args(parser, args):
    if args.data_format != "npy":
        return
    if args.data_on_device == "0":
        parser.error("--data_format npy lives on the device: it cannot run with --data_on_device 0")
    if args.image_size < 1:
        parser.error("--image_size must be at least 1")
    if not (math.isfinite(args.eval_crop) and 0 < args.eval_crop <= 1):
        parser.error("--eval_crop must lie in (0, 1]")
    try:
        rrc_config(args)
    except ValueError as e:
        parser.error(f"--rrc_scale / --rrc_ratio: {e}")


def rrc_config(args) -> RrcConfig:
    return RrcConfig(scale=tuple(args.rrc_scale), ratio=tuple(args.rrc_ratio))


def norm_of(args):
    """(mean, std) of --norm, which follows the data format when it is not given."""
    name = getattr(args, "norm", None) or ("imagenet" if getattr(args, "data_format", "cifar10") == "npy" else "cifar")
    return (IMAGENET_MEAN, IMAGENET_STD) if name == "imagenet" else (CIFAR_MEAN, CIFAR_STD)


def input_side(args) -> int:
    """The side of the step's input images: --image_size for synthetic and npy data, CIFAR's 32 otherwise."""
    resized = getattr(args, "synthetic", False) or getattr(args, "data_format", "cifar10") == "npy"
    return args.image_size if resized else 32


def add_recipe_args(p):
    """Label smoothing and mixup / CutMix (data/mix.py): the regularisers of the large-batch recipe."""
    p.add_argument("--label_smoothing", type=float, default=0.0, help="label smoothing of the training loss, in [0, 1)")
    p.add_argument("--mixup_alpha", type=float, default=0.0, help="mixup with lam ~ Beta(a, a) per batch (0 = off)")
    p.add_argument("--cutmix_alpha", type=float, default=0.0, help="CutMix with lam ~ Beta(a, a) per batch (0 = off)")
    p.add_argument("--mix_prob", type=float, default=1.0, help="probability that a batch is mixed at all")
    p.add_argument("--mix_switch_prob", type=float, default=0.5,
                   help="with both alphas > 0: probability that a mixed batch is CutMix rather than mixup")


def check_recipe_args(parser, args):
    if not (math.isfinite(args.label_smoothing) and 0 <= args.label_smoothing < 1):
        parser.error("--label_smoothing must lie in [0, 1)")
    for name in ("mixup_alpha", "cutmix_alpha"):
        v = getattr(args, name)
        if not (math.isfinite(v) and v >= 0):
            parser.error(f"--{name} must be finite and >= 0")
    for name in ("mix_prob", "mix_switch_prob"):
        if not 0 <= getattr(args, name) <= 1:
            parser.error(f"--{name} must lie in [0, 1]")


def recipe_of(args):
    """The mix configuration when any recipe flag is set, else None (then the step is built as without them)."""
    cfg = MixConfig(getattr(args, "mixup_alpha", 0.0), getattr(args, "cutmix_alpha", 0.0),
                    getattr(args, "mix_prob", 1.0), getattr(args, "mix_switch_prob", 0.5))
    return cfg if (getattr(args, "label_smoothing", 0.0) > 0 or cfg.enabled) else None


def add_layerwise_args(p, plain: str, layerwise: str):
    """--optimizer and the flags that only the layer-wise optimizer (LARS / LAMB) takes."""
    p.add_argument("--optimizer", default=plain, choices=[plain, layerwise],
                   help=f"{layerwise}: layer-wise trust ratios for a large global batch (no weight decay or "
                        "adaptation for BatchNorm and bias parameters)")
    p.add_argument("--lr_schedule", default=None, choices=["constant", "cosine", "poly"],
                   help=f"learning-rate schedule, evaluated on the device ({layerwise} only; default constant)")
    p.add_argument("--warmup_steps", type=int, default=None, help=f"linear warm-up updates ({layerwise} only)")
    p.add_argument("--trust_coefficient", type=float, default=1e-3, help="trust coefficient of LARS (LAMB's ratio has none)")


def check_layerwise_args(parser, args, plain: str):
    if args.optimizer == plain and (args.lr_schedule is not None or args.warmup_steps is not None):
        parser.error(f"--lr_schedule / --warmup_steps need the layer-wise optimizer, not --optimizer {plain}")
    if args.warmup_steps is not None and args.warmup_steps < 0:
        parser.error("--warmup_steps must be >= 0")


def schedule_of(args, total_steps: int) -> dict:
    return dict(kind=args.lr_schedule or "constant", warmup_steps=args.warmup_steps or 0,
                total_steps=max(1, int(total_steps)))


def use_graph(args, device, pixels=None, comm_backend="single") -> bool:
    """--graph auto: capture the step when it is launch-bound -- native bf16 kernels on a GPU and a
    step smaller than the auxiliary-stream threshold (N*H*W < DLMPI_AUX_MIN_PIXELS, default 1M:
    the reference's ResNet-18 on CIFAR, 46k -> 85k img/s).  Larger steps run their weight-gradient
    and residual-branch streams concurrently, which a replayed graph loses (measured: ResNet-50
    bs 256 -7 %, ResNet-152 -13 %, UNet 512 -2 %, profiles/r2_graph_ab).  Auto mode also requires a
    capturable data plane: RCCL (device collectives on the comm stream) or a single rank -- gloo's
    host-staged collectives (the DLMPI_GLOO_DEVICE=cuda rehearsal) cannot live inside a hipGraph."""
    if args.graph in (True, "1"):
        return device.type == "cuda"
    if args.graph in (False, "0"):
        return False
    if device.type != "cuda" or comm_backend not in ("rccl", "single"):
        return False
    if pixels is None:
        pixels = args.batch_size * input_side(args) ** 2
    return pixels < int(os.environ.get("DLMPI_AUX_MIN_PIXELS", str(1 << 20)))


def set_random_seeds(seed: int):
    """Seeds + the reference's cuDNN flags (C16: resnet/main.py:26-33, unet/train.py:35-41).  The
    flags only affect stock torch ops; the engine's own kernels are deterministic by construction
    (fixed-order reductions, no float atomics; the bilinear up-sampling backward is a gather)."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = True


@torch.no_grad()
def evaluate(model, device, test_loader) -> float:
    model.eval()
    correct = torch.zeros(1, dtype=torch.int64, device=device)
    total = 0
    for images, labels in test_loader:
        images, labels = images.to(device, non_blocking=True), labels.to(device, non_blocking=True)
        correct += top1_correct(model(images), labels).to(torch.int64)
        total += labels.size(0)
    model.train()
    return correct.item() / max(1, total)


def build_loaders(args, device, static, mix_cfg):
    """-> (train_set, sampler, train_loader, test_loader) of the run; ``static``: the captured step's inputs, which
    a device-resident training loader fills in place under --graph."""
    npy = getattr(args, "data_format", "cifar10") == "npy" and not args.synthetic
    on_device = (npy or args.data_on_device == "1" or
                 (args.data_on_device == "auto" and device.type == "cuda" and not args.synthetic))
    test_bs = args.test_batch_size or args.batch_size
    side = input_side(args)
    mean, std = norm_of(args)
    # the CIFAR loaders take their constants only when --norm names them: by default they are built as ever
    norm = dict(mean=mean, std=std) if getattr(args, "norm", None) else {}
    if args.synthetic:
        shape = (3, args.image_size, args.image_size)
        train_set = SyntheticImages(args.synthetic_size, shape, args.num_classes, seed=1)
        test_set = SyntheticImages(max(64, args.synthetic_size // 8), shape, args.num_classes, seed=2)
    elif npy:
        # images of any stored size in HBM; one kernel per batch does gather + RandomResizedCrop + flip + normalize
        # into [B, 3, S, S]; a mix is applied to the finished batch (step_inputs), as for any unmixed loader
        train_set = DeviceImageDataset.from_npy(args.data_root, "train", device, mean=mean, std=std,
                                                seed=args.random_seed, rrc=rrc_config(args), out_size=side)
        test_set = DeviceImageDataset.from_npy(args.data_root, "val", device, mean=mean, std=std,
                                               eval_crop=args.eval_crop, out_size=side)
    elif on_device:
        # the whole dataset in HBM; one kernel per batch does gather + crop/flip + normalize
        train_set = DeviceImageDataset.cifar10(args.data_root, True, device, seed=args.random_seed, mix=mix_cfg,
                                               **norm)
        test_set = DeviceImageDataset.cifar10(args.data_root, False, device, augment=False, **norm)
    else:
        # download=False semantics: the data must already be under data_root (see download.py)
        # augmentation = f(seed, epoch, index) (data/datasets.py SampleRng): rank-, worker- and
        # resume-independent
        train_set = CIFAR10(args.data_root, train=True, transform=CifarTransform(True, **norm), seed=args.random_seed)
        test_set = CIFAR10(args.data_root, train=False, transform=CifarTransform(False, **norm))
    sampler = DistributedSampler(train_set, seed=0)
    if on_device and not args.synthetic:
        train_loader = DeviceBatches(train_set, args.batch_size, sampler,
                                     out=static if args.graph else None)
        test_loader = DeviceBatches(test_set, test_bs)
    else:
        pin = device.type == "cuda"
        # workers are re-created every epoch (reference default) so they see the dataset's epoch
        train_loader = DataLoader(train_set, batch_size=args.batch_size, sampler=sampler, num_workers=args.workers,
                                  pin_memory=pin)
        # a private generator: rank-0-only evaluation must not advance the global host RNG (its
        # state is the resume state every rank restores)
        test_loader = DataLoader(test_set, batch_size=test_bs, shuffle=False, num_workers=args.workers,
                                 pin_memory=pin, generator=torch.Generator().manual_seed(args.random_seed))
    return train_set, sampler, train_loader, test_loader


def run(args) -> dict:
    comm = parallel.init_distributed(args.backend)
    rank, world, local_rank = comm.rank, comm.world_size, comm.local_rank
    device = comm.device if args.device == "auto" else torch.device(args.device)
    set_random_seeds(args.random_seed)
    model = ARCHS[args.arch](num_classes=args.num_classes).to(device)
    model.precision = args.precision
    ddp = parallel.DistributedDataParallel(model, bucket_cap_mb=args.bucket_mb)
    model_filepath = os.path.join(args.model_dir, args.model_filename)
    args.graph = use_graph(args, device, comm_backend=getattr(comm, "backend", "single"))

    # the training step reads its batch from fixed tensors so that it can be captured (--graph)
    side = input_side(args)
    x_static = torch.empty((args.batch_size, 3, side, side), device=device)
    y_static = torch.zeros(args.batch_size, dtype=torch.int64, device=device)
    static = (x_static, y_static)
    mix_cfg = recipe_of(args)
    if mix_cfg is not None:   # the step reads a mixed target: (x, labels_a, labels_b, lam), all on the device
        static += (torch.zeros_like(y_static), torch.ones(1, dtype=torch.float32, device=device))
    train_set, sampler, train_loader, test_loader = build_loaders(args, device, static, mix_cfg)
    criterion = CrossEntropyLoss(label_smoothing=getattr(args, "label_smoothing", 0.0))
    if getattr(args, "optimizer", "sgd") == "lars":
        steps = args.benchmark_steps or args.num_epochs * (args.steps_per_epoch or len(train_loader))
        optimizer = LARS(model.parameters(), lr=args.learning_rate, momentum=0.9, weight_decay=1e-5,
                         trust_coefficient=args.trust_coefficient, schedule=schedule_of(args, steps))
    else:
        optimizer = SGD(model.parameters(), lr=args.learning_rate, momentum=0.9, weight_decay=1e-5)
    start_epoch = 0
    if args.resume:
        # weights (reference layout) + the sidecar: optimizer state, next epoch, RNG states
        meta = load_checkpoint(ddp, model_filepath, map_location=device, optimizer=optimizer)
        start_epoch = int(meta.get("next_epoch", 0))
        set_rng_state(meta.get("rng"))
    ema = ema_of(args, ddp, optimizer)   # (a copy of the weights as they are now: the loaded ones on --resume)
    if ema is not None and args.resume and "ema" in meta:
        ema.load_state_dict(meta["ema"])   # after the optimizer's: the step counter it last saw is the restored one

    def train_step(x, y, y_b=None, lam=None):
        optimizer.zero_grad()
        loss = criterion(ddp(x), y) if y_b is None else criterion(ddp(x), y, y_b, lam)
        backward(loss)
        optimizer.step()
        if ema is not None:
            ema.update()
        return loss

    captured = None
    if args.graph and device.type == "cuda":
        captured = CapturedStep(lambda: train_step(*static), warmup=2, inputs=static, comm=comm)

    if args.benchmark_steps:
        return benchmark(args, train_step, captured, static, comm, device, mix_cfg)

    def step_inputs(batch, epoch, batch_no):
        """The batch on the device as the step takes it.  With the recipe flags a batch that the loader has not
        mixed already (DataLoader, synthetic) is mixed in place here, outside the captured step -- a full batch
        inside the step's fixed tensors."""
        batch = tuple(t.to(device, non_blocking=True) for t in batch)
        if mix_cfg is None or len(batch) == 4:
            return batch
        x, y = batch
        p = draw_mix(mix_cfg, args.random_seed, epoch, rank, batch_no, x.shape[2], x.shape[3])
        if captured is not None and x.shape[0] == args.batch_size:
            captured.set_inputs(x, y)
            return mix_batch_(static[0], static[1], p, static[2], static[3])
        return mix_batch_(x.contiguous(), y, p)

    history = {"loss": [], "accuracy": [], "images_per_sec": []}

    def eval_and_save(epoch, next_epoch):
        state = resume_state(next_epoch)   # RNG states of the epoch boundary, taken before evaluating
        accuracy = evaluate(model, device, test_loader)
        if ema is not None:
            state["ema"] = ema.state_dict()
        save_checkpoint(ddp, model_filepath, optimizer=optimizer, extra=state, rank=rank)
        print("-" * 75)
        print("Epoch: {}, Accuracy: {}".format(epoch, accuracy))
        print("-" * 75)
        history["accuracy"].append(accuracy)
        if ema is not None:
            with ema.applied():   # the model holds the averaged weights and BN statistics
                ema_accuracy = evaluate(model, device, test_loader)
                save_checkpoint(ddp, ema_path(model_filepath), rank=rank)   # reference layout, atomic, rank 0
            print("Epoch: {}, EMA Accuracy: {}".format(epoch, ema_accuracy))
            print("-" * 75)
            history.setdefault("ema_accuracy", []).append(ema_accuracy)

    try:
        for epoch in range(start_epoch, args.num_epochs):
            sampler.set_epoch(epoch)
            if hasattr(train_set, "set_epoch"):
                train_set.set_epoch(epoch)
            if args.eval_before_train and epoch % args.eval_every == 0 and rank == 0:
                eval_and_save(epoch, epoch)
            print("Local Rank: {}, Epoch: {}, Training ...".format(local_rank, epoch))
            ddp.train()
            loss_sum = torch.zeros((), device=device)
            nb = 0
            t0 = time.perf_counter()
            for batch in train_loader:
                batch = step_inputs(batch, epoch, nb)
                if captured is not None and batch[0].shape[0] == args.batch_size:
                    captured.set_inputs(*batch)
                    loss = captured()
                else:   # eager step (also the ragged last batch of a graph run)
                    loss = train_step(*batch)
                loss_sum += loss.detach()
                nb += 1
                if args.steps_per_epoch and nb >= args.steps_per_epoch:
                    break
            mean_loss = (loss_sum / max(1, nb)).item()
            dt = time.perf_counter() - t0
            history["loss"].append(mean_loss)
            history["images_per_sec"].append(nb * args.batch_size * world / dt)
            print("Local Rank: {}, Epoch: {}, Loss: {}".format(local_rank, epoch, mean_loss))
            if rank == 0:
                print(f"Epoch {epoch} throughput: {history['images_per_sec'][-1]:.1f} images/sec ({nb} steps)")
            if not args.eval_before_train and epoch % args.eval_every == 0 and rank == 0:
                eval_and_save(epoch, epoch + 1)
            print(f"Epoch {epoch} completed")
    finally:
        parallel.destroy_distributed()
    return history


def benchmark(args, train_step, captured, static, comm, device, mix_cfg=None) -> dict:
    """--benchmark_steps: synthetic device batch, 3 warm-up steps, timed steps, images/sec.  With the recipe flags
    a timed step is the in-place mix of the batch plus the training step."""
    x, y = static[:2]
    g = torch.Generator(device=device).manual_seed(1234 + comm.rank)
    x.copy_(torch.randn(x.shape, generator=g, device=device))
    y.copy_(torch.randint(args.num_classes, y.shape, generator=g, device=device))
    run_step = captured if captured is not None else (lambda: train_step(*static))
    if mix_cfg is None:
        step = lambda i: run_step()   # noqa: E731
    else:
        def step(i):
            p = draw_mix(mix_cfg, args.random_seed, 0, comm.rank, i, x.shape[2], x.shape[3])
            mix_batch_(x, y, p, static[2], static[3])
            return run_step()
    for i in range(3):
        step(i)
    comm.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.benchmark_steps):
        loss = step(3 + i)
    comm.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ips = args.batch_size * comm.world_size * args.benchmark_steps / dt
    if comm.rank == 0:
        print(f"benchmark: {args.arch} bs={args.batch_size}/rank x {comm.world_size} ranks, "
              f"{args.benchmark_steps} steps: {ips:.1f} images/sec ({dt / args.benchmark_steps * 1e3:.2f} ms/step), "
              f"loss {float(loss.detach()):.4f}")
    parallel.destroy_distributed()
    return {"images_per_sec": ips}


def main(variant="main", argv=None):
    parser = build_argparser(variant)
    args = parser.parse_args(argv)
    check_layerwise_args(parser, args, "sgd")
    check_recipe_args(parser, args)
    check_data_args(parser, args)
    check_ema_args(parser, args)
    return run(args)
