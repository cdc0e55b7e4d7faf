"""UNet data-parallel segmentation training (the reference's pytorch/unet/train.py).

Same flags/defaults (--num_epochs 100, --batch_size 16, --learning_rate 1e-4, --random_seed 42,
--model_dir saved_models, --model_filename model.pth, --resume), same log file
(logs/training_log_YYYYmmdd_HHMMSS.log: header, "Started training at", per-epoch
"Epoch e | Loss: x | Duration: s", every 10 epochs "Epoch e | Dice Score: x", final block) and the
same Adam + BCEWithLogits + clip_grad_norm_(1.0) step (/root/reference/pytorch/unet/train.py:143-244).

Deliberate fixes: the NaN/Inf skip is collective (decided from the
all-reduced gradient norm on the device, identical on every rank -> no deadlock, no host sync);
the log and checkpoints are written by global rank 0 only; evaluation uses the unwrapped module.
Additions: --synthetic, --image_size, --in_channels, --data_dir, --scale, --up_sample_mode,
--backend, --device, --max_norm, --steps_per_epoch, --workers, and multi-class masks: --num_classes K > 1
trains UNet(out_classes=K) on the integer class-index masks with the pixel-wise CrossEntropyLoss
(--ignore_index) and evaluates the mean foreground Dice of the argmax (ops.dice_multiclass).
--loss {ce,dice,ce+dice} (default ce: the criteria above) trains on the differentiable soft Dice as well:
sigmoid form for --num_classes 1, softmax form for K > 1 (ops.bce_dice_loss / ce_dice_loss / dice_loss;
--dice_weight, --dice_smooth, --dice_background 0 to leave class 0 out of the mean).  On the GPU the Dice
sums and gradient ride in the cross-entropy kernels' passes: one forward, one finish, one backward.
--aug_hflip / --aug_vflip / --aug_scale / --aug_rotate / --aug_translate / --aug_prob (defaults: none) augment
the training split on the device: the pairs stay resident and one kernel per batch gathers and resamples image
and mask (data/seg_aug.py, DeviceSegDataset); evaluation is unchanged.
"""
from __future__ import annotations

import argparse
import os
import sys
import random
import time
from datetime import datetime

import numpy as np
import torch
from torch.utils.data import DataLoader
from tqdm import tqdm

from .. import parallel
from ..data import (CarvanaDataset, DeviceBatches, DeviceCachedDataset, DeviceSegDataset, DistributedSampler,
                    SegAugConfig, SyntheticMasks)
from ..models import UNet
from ..ops import (BCEDiceLoss, BCEWithLogitsLoss, CEDiceLoss, CrossEntropyLoss, DiceLoss, backward, dice_multiclass,
                   dice_per_sample)
from ..optim import LAMB, Adam, clip_grad_norm_
from ..utils.graphs import CapturedStep
from ..utils.checkpoint import load_checkpoint, resume_state, save_checkpoint, set_rng_state
from .classification import (add_ema_args, add_layerwise_args, check_ema_args, check_layerwise_args, ema_of, ema_path,
                             schedule_of, use_graph)


def build_argparser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--num_epochs", type=int, default=100, help="Number of training epochs.")
    p.add_argument("--batch_size", type=int, default=16, help="Batch size per process.")
    p.add_argument("--learning_rate", type=float, default=0.0001, help="Learning rate.")
    p.add_argument("--random_seed", type=int, default=42, help="Seed for reproducibility.")
    p.add_argument("--model_dir", type=str, default="saved_models", help="Directory to save model.")
    p.add_argument("--model_filename", type=str, default="model.pth", help="Model filename.")
    p.add_argument("--resume", action="store_true", help="Resume from a checkpoint.")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--synthetic_size", type=int, default=64)
    p.add_argument("--image_size", type=int, default=512)
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=1,
                   help="1: one logit per pixel, BCEWithLogits on the binarised mask (the reference); K > 1: K "
                        "logits per pixel, pixel-wise cross-entropy on the mask's class indices")
    p.add_argument("--ignore_index", type=int, default=-100,
                   help="label left out of the multi-class loss and Dice (--num_classes > 1)")
    p.add_argument("--loss", default="ce", choices=["ce", "dice", "ce+dice"],
                   help="ce: BCEWithLogits (--num_classes 1) / pixel-wise cross-entropy (K > 1); dice: the soft Dice "
                        "loss of sigmoid / softmax; ce+dice: their sum, computed in the passes of ce alone")
    p.add_argument("--dice_weight", type=float, default=1.0, help="weight of the Dice term (--loss ce+dice)")
    p.add_argument("--dice_smooth", type=float, default=1.0, help="smoothing constant of the soft Dice (> 0)")
    p.add_argument("--dice_background", type=int, default=1, choices=[0, 1],
                   help="0: leave class 0 out of the multi-class Dice mean")
    p.add_argument("--data_dir", default="data")
    p.add_argument("--scale", type=float, default=0.2)
    p.add_argument("--up_sample_mode", default="conv_transpose", choices=["conv_transpose", "bilinear"])
    p.add_argument("--backend", default="nccl")
    p.add_argument("--device", default="auto")
    p.add_argument("--max_norm", type=float, default=1.0)
    p.add_argument("--steps_per_epoch", type=int, default=0)
    p.add_argument("--workers", type=int, default=max(1, (os.cpu_count() or 2) // 2))
    p.add_argument("--data_on_device", default="auto", choices=["auto", "0", "1"],
                   help="decode the dataset once and keep it in GPU memory; batches are device-side gathers "
                        "(auto: on for GPU runs when it needs < 1/4 of the GPU memory)")
    p.add_argument("--log_dir", default="logs")
    p.add_argument("--eval_every", type=int, default=10)
    p.add_argument("--bucket_mb", type=float, default=None)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32"],
                   help="bf16: native gfx950 kernels on bf16 activations; fp32: the same kernels on fp32 "
                        "activations and weights (fp32 MFMA)")
    p.add_argument("--graph", nargs="?", const="1", default="auto", choices=["auto", "0", "1"],
                   help="replay each full-size training step from a captured hipGraph (ragged last batches run "
                        "eagerly); auto = on for launch-bound GPU training")
    p.add_argument("--benchmark_steps", type=int, default=0,
                   help="time this many steps on a synthetic device batch, print images/sec and exit")
    p.add_argument("--aug_hflip", type=float, default=0.0, help="probability of a horizontal flip of a training sample")
    p.add_argument("--aug_vflip", type=float, default=0.0, help="probability of a vertical flip")
    p.add_argument("--aug_scale", type=float, nargs=2, default=[1.0, 1.0], metavar=("LO", "HI"),
                   help="isotropic zoom, log-uniform in [LO, HI]")
    p.add_argument("--aug_rotate", type=float, default=0.0, help="rotation uniform in +-DEG degrees")
    p.add_argument("--aug_translate", type=float, default=0.0,
                   help="translation uniform in +-F of the image width / height")
    p.add_argument("--aug_prob", type=float, default=1.0,
                   help="probability that a sample gets its scale / rotation / translation (flips are drawn apart)")
    add_layerwise_args(p, "adam", "lamb")
    p.add_argument("--weight_decay", type=float, default=None,
                   help="weight decay (default: 0 for adam, 0.01 for lamb)")
    add_ema_args(p)
    return p


def set_random_seeds(seed):
    """Seeds + the reference's cuDNN flags (C16: resnet/main.py:26-33, unet/train.py:35-41).  The
    flags only affect stock torch ops; the engine's own kernels are deterministic by construction
    (fixed-order reductions, no float atomics; the bilinear up-sampling backward is a gather)."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = True


def create_log_file(log_dir="logs") -> str:
    return os.path.join(log_dir, f"training_log_{datetime.now().strftime('%Y%m%d_%H%M%S')}.log")


class RankLog:
    def __init__(self, path, rank):
        self.path, self.rank = path, rank
        if rank == 0 and path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)

    def __call__(self, msg):
        if self.rank == 0 and self.path:
            with open(self.path, "a") as f:
                f.write(msg + "\n")


@torch.no_grad()
def evaluate_model(model, device, test_loader, num_classes=1, ignore_index=-100) -> float:
    model.eval()
    scores = []
    for batch in test_loader:
        images = batch["image"].to(device, dtype=torch.float32)
        if num_classes > 1:
            masks = batch["mask"].to(device, dtype=torch.int64)
            scores.append(dice_multiclass(model(images), masks, ignore_index))
        else:
            masks = batch["mask"].to(device, dtype=torch.float32)
            scores.append(dice_per_sample(model(images), masks))
    model.train()
    if not scores:
        return 0.0
    return torch.cat(scores).mean().item()


def seg_aug_config(args) -> SegAugConfig:
    """The --aug_* flags (absent on namespaces that callers build themselves: the defaults, no augmentation)."""
    return SegAugConfig(hflip=getattr(args, "aug_hflip", 0.0), vflip=getattr(args, "aug_vflip", 0.0),
                        scale=tuple(getattr(args, "aug_scale", (1.0, 1.0))), rotate=getattr(args, "aug_rotate", 0.0),
                        translate=getattr(args, "aug_translate", 0.0), prob=getattr(args, "aug_prob", 1.0))


def build_data_loaders(args, device):
    if args.synthetic:
        ds = SyntheticMasks(args.synthetic_size, (args.in_channels, args.image_size, args.image_size),
                            seed=args.random_seed, num_classes=args.num_classes)
    else:
        ds = CarvanaDataset(images_dir=os.path.join(args.data_dir, "images"),
                            mask_dir=os.path.join(args.data_dir, "masks"), scale=args.scale,
                            multiclass=args.num_classes > 1)
        if args.num_classes > 1 and len(ds.mask_values) > args.num_classes:
            raise ValueError(f"the masks under {args.data_dir} hold {len(ds.mask_values)} distinct values, more "
                             f"than --num_classes {args.num_classes}")
    train_size = int(0.8 * len(ds))
    test_size = len(ds) - train_size
    # same split on every rank (seeded generator rather than the global RNG)
    train_ds, test_ds = torch.utils.data.random_split(ds, [train_size, test_size],
                                                      generator=torch.Generator().manual_seed(args.random_seed))
    aug = seg_aug_config(args)
    if aug.enabled:
        # geometric augmentation of the training split: the pairs stay in device memory and one kernel per batch
        # gathers and resamples them (evaluation is untouched); outside the source the multi-class mask carries
        # --ignore_index, which the losses and the Dice counts leave out
        if args.data_on_device == "0":
            raise ValueError("the --aug_* flags augment on the device: they cannot go with --data_on_device 0")
        train_c = DeviceSegDataset(train_ds, device, aug, seed=args.random_seed,
                                   mask_fill=args.ignore_index if args.num_classes > 1 else 0.0)
        test_c = DeviceCachedDataset(test_ds, device)
        sampler = DistributedSampler(train_c)
        return DeviceBatches(train_c, args.batch_size, sampler), DeviceBatches(test_c, args.batch_size), sampler
    if _use_device_data(args, device, ds):
        # the reference dataset is deterministic (no augmentation): decode / resize once, keep the
        # tensors in HBM, and serve every batch as an index gather on the device
        train_c, test_c = DeviceCachedDataset(train_ds, device), DeviceCachedDataset(test_ds, device)
        sampler = DistributedSampler(train_c)
        return DeviceBatches(train_c, args.batch_size, sampler), DeviceBatches(test_c, args.batch_size), sampler
    kw = dict(batch_size=args.batch_size, num_workers=args.workers, pin_memory=device.type == "cuda")
    sampler = DistributedSampler(train_ds)
    # evaluation runs on rank 0 only: its loader gets a private generator so it never advances the
    # global host RNG that every rank restores on --resume
    return (DataLoader(train_ds, sampler=sampler, **kw),
            DataLoader(test_ds, shuffle=False, generator=torch.Generator().manual_seed(args.random_seed), **kw),
            sampler)


def _use_device_data(args, device, ds) -> bool:
    """--data_on_device auto: on for GPU runs whose decoded dataset needs < 1/4 of the GPU memory."""
    if args.data_on_device != "auto":
        return args.data_on_device == "1"
    if device.type != "cuda":
        return False
    s = ds[0]
    per = sum(torch.as_tensor(v).numel() * 4 for v in s.values())
    return per * len(ds) < torch.cuda.get_device_properties(device).total_memory // 4


def benchmark(args, train_step, captured, x, y, comm, device) -> dict:
    """--benchmark_steps: synthetic device batch, 3 warm-up steps, timed steps, images/sec."""
    g = torch.Generator(device=device).manual_seed(1234 + comm.rank)
    x.copy_(torch.randn(x.shape, generator=g, device=device))
    if args.num_classes > 1:
        y.copy_(torch.randint(args.num_classes, y.shape, generator=g, device=device))
    else:
        y.copy_((torch.rand(y.shape, generator=g, device=device) > 0.5).float())
    step = captured if captured is not None else (lambda: train_step(x, y))
    for _ in range(3):
        step()
    comm.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.benchmark_steps):
        loss = step()
    comm.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ips = args.batch_size * comm.world_size * args.benchmark_steps / dt
    if comm.rank == 0:
        print(f"benchmark: UNet {args.in_channels}x{args.image_size}^2 bs={args.batch_size}/rank x {comm.world_size} "
              f"ranks, {args.benchmark_steps} steps: {ips:.2f} images/sec ({dt / args.benchmark_steps * 1e3:.1f} "
              f"ms/step), loss {float(loss.detach()):.4f}")
    parallel.destroy_distributed()
    return {"images_per_sec": ips}


def build_criterion(args):
    """--loss ce (the default): today's BCEWithLogitsLoss / CrossEntropyLoss; dice, ce+dice: the fused soft
    Dice losses, sigmoid form for --num_classes 1, softmax form (honouring --ignore_index) for K > 1."""
    K = args.num_classes
    kind = getattr(args, "loss", "ce")   # (callers that build the namespace themselves)
    if kind == "ce":
        return CrossEntropyLoss(ignore_index=args.ignore_index) if K > 1 else BCEWithLogitsLoss()
    if kind not in ("dice", "ce+dice"):
        raise ValueError(f"--loss must be ce, dice or ce+dice, got {kind!r}")
    smooth = getattr(args, "dice_smooth", 1.0)
    if kind == "dice":
        if K > 1:
            return DiceLoss(smooth=smooth, include_background=bool(getattr(args, "dice_background", 1)),
                            ignore_index=args.ignore_index)
        return DiceLoss(smooth=smooth)
    dw = getattr(args, "dice_weight", 1.0)
    if K > 1:
        return CEDiceLoss(ignore_index=args.ignore_index, dice_weight=dw, smooth=smooth,
                          include_background=bool(getattr(args, "dice_background", 1)))
    return BCEDiceLoss(dice_weight=dw, smooth=smooth)


def run(args) -> dict:
    if args.num_classes < 1:   # (callers that build the namespace themselves)
        raise ValueError(f"--num_classes must be >= 1, got {args.num_classes}")
    comm = parallel.init_distributed(args.backend)
    rank, world, local_rank = comm.rank, comm.world_size, comm.local_rank
    device = comm.device if args.device == "auto" else torch.device(args.device)
    set_random_seeds(args.random_seed)
    log = RankLog(create_log_file(args.log_dir), rank)
    gpu = torch.cuda.get_device_name(device) if device.type == "cuda" else "cpu"
    log(f"Batch size: {args.batch_size}")
    log(f"Number of workers: {os.cpu_count()}")
    log(f"Learning rate: {args.learning_rate}")
    log(f"Number of epochs: {args.num_epochs}")
    log(f"World size: {world}, Local rank: {local_rank}, GPU: {gpu}")

    train_loader, test_loader, sampler = build_data_loaders(args, device)
    K = args.num_classes
    mask_dtype = torch.int64 if K > 1 else torch.float32
    model = UNet(out_classes=K, up_sample_mode=args.up_sample_mode, in_channels=args.in_channels).to(device)
    model.precision = args.precision
    ddp = parallel.DistributedDataParallel(model, bucket_cap_mb=args.bucket_mb)
    model_filepath = os.path.join(args.model_dir, args.model_filename)
    wd = getattr(args, "weight_decay", None)
    if getattr(args, "optimizer", "adam") == "lamb":
        steps = args.benchmark_steps or args.num_epochs * (args.steps_per_epoch or len(train_loader))
        optimizer = LAMB(model.parameters(), lr=args.learning_rate, weight_decay=0.01 if wd is None else wd,
                         schedule=schedule_of(args, steps))
    else:
        optimizer = Adam(model.parameters(), lr=args.learning_rate, weight_decay=wd or 0.0)
    criterion = build_criterion(args)
    start_epoch = 0
    if args.resume:
        # weights (reference layout) + the sidecar: Adam moments and step, next epoch, RNG states
        meta = load_checkpoint(ddp, model_filepath, map_location=device, optimizer=optimizer)
        start_epoch = int(meta.get("next_epoch", 0))
        set_rng_state(meta.get("rng"))
    # averaged weights (--ema_decay): the optimizer's device step counter tells a skipped update (the clip hand-off's
    # non-finite norm) from an applied one
    ema = ema_of(args, ddp, optimizer)
    if ema is not None and args.resume and "ema" in meta:
        ema.load_state_dict(meta["ema"])   # after the optimizer's
    args.graph = use_graph(args, device, pixels=args.batch_size * args.image_size * args.image_size,
                           comm_backend=getattr(comm, "backend", "single"))

    def train_step(images, masks):
        pred = ddp(images)
        if K == 1:
            pred = pred.squeeze(1)
        loss = criterion(pred, masks)
        optimizer.zero_grad()
        backward(loss)
        # collective NaN/Inf guard: a non-finite all-reduced grad norm skips the step on all ranks
        clip_grad_norm_(model.parameters(), max_norm=args.max_norm, optimizer=optimizer)
        optimizer.step()
        if ema is not None:
            ema.update()
        return loss

    def save(state):
        if ema is not None:
            state["ema"] = ema.state_dict()
        save_checkpoint(ddp, model_filepath, optimizer=optimizer, extra=state, rank=rank)

    def ema_dice():
        """Dice of the averaged model; its weights go next to the trained ones in the reference's layout."""
        with ema.applied():
            d = evaluate_model(model, device, test_loader, K, args.ignore_index)
            save_checkpoint(ddp, ema_path(model_filepath), rank=rank)
        return d

    S = args.image_size
    x_static = torch.zeros(args.batch_size, args.in_channels, S, S, device=device)
    y_static = torch.zeros(args.batch_size, S, S, dtype=mask_dtype, device=device)
    captured = None
    if args.graph and device.type == "cuda":
        captured = CapturedStep(lambda: train_step(x_static, y_static), warmup=2, inputs=(x_static, y_static),
                                comm=comm)
        seg = getattr(train_loader, "ds", None)
        if isinstance(seg, DeviceSegDataset) and (seg.C, seg.Ho, seg.Wo) == tuple(x_static.shape[1:]):
            # the batch kernel writes full batches straight into the captured step's inputs (set_inputs then
            # has nothing to copy); it runs outside the captured graph
            train_loader.out = (x_static, y_static)
    if args.benchmark_steps:
        return benchmark(args, train_step, captured, x_static, y_static, comm, device)
    history = {"loss": [], "dice": []}
    if rank == 0:
        print(f"Logging training progress to: {log.path}")
    log(f"Started training at {datetime.now()}")
    try:
        for epoch in range(start_epoch, args.num_epochs):
            sampler.set_epoch(epoch)
            t0 = time.time()
            ddp.train()
            loss_sum = torch.zeros((), device=device)
            nb = 0
            bar = tqdm(train_loader, desc=f"Epoch {epoch + 1}/{args.num_epochs}", unit="batch",
                       disable=rank != 0 or not sys.stderr.isatty())   # no per-step host sync for a loss postfix
            for batch in bar:
                images = batch["image"].to(device, dtype=torch.float32, non_blocking=True)
                masks = batch["mask"].to(device, dtype=mask_dtype, non_blocking=True)
                if captured is not None and images.shape == x_static.shape:
                    captured.set_inputs(images, masks)
                    loss = captured()
                else:
                    loss = train_step(images, masks)
                loss_sum += torch.nan_to_num(loss.detach(), nan=0.0, posinf=0.0, neginf=0.0)
                nb += 1
                if args.steps_per_epoch and nb >= args.steps_per_epoch:
                    break
            avg_loss = (loss_sum / max(1, nb)).item()
            history["loss"].append(avg_loss)
            print(f"Epoch {epoch + 1} finished with loss: {avg_loss:.4f}")
            log(f"Epoch {epoch + 1} | Loss: {avg_loss:.4f} | Duration: {time.time() - t0:.2f}s")
            if (epoch + 1) % args.eval_every == 0 and rank == 0:
                state = resume_state(epoch + 1)   # epoch-boundary RNG states, taken before evaluating
                dice = evaluate_model(model, device, test_loader, K, args.ignore_index)
                save(state)
                print("-" * 75)
                print(f"Epoch {epoch + 1} Dice Score: {dice:.4f}")
                print("-" * 75)
                log(f"Epoch {epoch + 1} | Dice Score: {dice:.4f}")
                history["dice"].append(dice)
                if ema is not None:
                    d = ema_dice()
                    print(f"Epoch {epoch + 1} EMA Dice Score: {d:.4f}")
                    print("-" * 75)
                    log(f"Epoch {epoch + 1} | EMA Dice Score: {d:.4f}")
                    history.setdefault("ema_dice", []).append(d)
        if rank == 0:
            print("\n" + "=" * 80 + "\nTRAINING COMPLETED - FINAL EVALUATION\n" + "=" * 80)
            state = resume_state(args.num_epochs)
            final = evaluate_model(model, device, test_loader, K, args.ignore_index)
            save(state)
            print(f"FINAL DICE COEFFICIENT: {final:.4f}\n" + "=" * 80 + "\n")
            log("=" * 80)
            log("FINAL TRAINING RESULTS")
            log("=" * 80)
            log(f"TRAINING COMPLETED | Final Dice Coefficient: {final:.4f} | Training finished at: {datetime.now()}")
            log(f"Total training epochs: {args.num_epochs}")
            log(f"Final learning rate: {args.learning_rate}")
            log(f"Model saved to: {model_filepath}")
            log("=" * 80)
            history["final_dice"] = final
            if ema is not None:
                history["final_ema_dice"] = ema_dice()
                print(f"FINAL EMA DICE COEFFICIENT: {history['final_ema_dice']:.4f}")
                log(f"Final EMA Dice Coefficient: {history['final_ema_dice']:.4f}")
    finally:
        parallel.destroy_distributed()
    return history


def parse_args(argv=None):
    p = build_argparser()
    args = p.parse_args(argv)
    if args.num_classes < 1:
        p.error(f"--num_classes must be >= 1, got {args.num_classes}")
    check_layerwise_args(p, args, "adam")
    check_ema_args(p, args)
    try:
        aug = seg_aug_config(args)
    except ValueError as e:
        p.error(f"--aug_*: {e}")
    if aug.enabled and args.data_on_device == "0":
        p.error("the --aug_* flags augment on the device: they cannot go with --data_on_device 0")
    return args


def main(argv=None):
    return run(parse_args(argv))
