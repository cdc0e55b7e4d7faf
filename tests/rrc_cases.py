"""Sources, hand-written crop tables and the fp64 yardstick shared by tests/test_rrc_cpu.py and
tests/test_rrc_gpu.py.

A group is one kernel launch: a source of four images, an output size and a table of four boxes; ``IDX`` gathers
five samples from it, one twice and not in ascending order.  The boxes are the edge cases of the resampling: the
whole image, a single pixel, a 33 x 3 sliver, a box that touches the bottom-right corner, an up-scale, and a
down-scale by more than 9 on a 64-wide source (21 taps per output pixel).  ``Wo`` = 24 and 16 take the kernel's
16-byte store path, 9 and 7 the scalar one."""
import os

import numpy as np
import torch
import torch.nn.functional as F

MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
IDX = [3, 2, 2, 0, 1]

# name: ((H, W) of the source, (Ho, Wo), rows (top, left, h, w, flip))
GROUPS = {
    "to16x24": ((37, 41), (16, 24), [(0, 0, 37, 41, 0), (2, 30, 33, 3, 0), (0, 0, 37, 41, 1), (10, 12, 7, 5, 1)]),
    "to7x9": ((37, 41), (7, 9), [(0, 0, 37, 41, 0), (5, 7, 1, 1, 0), (20, 25, 17, 16, 0), (20, 25, 17, 16, 1)]),
    "up16x16": ((37, 41), (16, 16), [(10, 12, 7, 5, 0), (10, 12, 7, 5, 1), (0, 0, 37, 41, 0), (21, 25, 16, 16, 0)]),
    "down9x": ((20, 64), (7, 7), [(0, 0, 20, 64, 0), (0, 0, 20, 64, 1), (0, 0, 20, 63, 1), (3, 1, 14, 60, 0)]),
}


def source(H, W, C=3, N=4, seed=0):
    """uint8 [N, H, W, C] noise (the hardest input of an averaging filter) and labels [N]."""
    g = np.random.default_rng([seed, H, W])
    return g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)[..., :C].copy(), np.arange(10, 10 + N, dtype=np.int64)


def table_of(rows):
    return np.array(rows, dtype=np.int32).reshape(-1, 5)


def yardstick(data, idx, table, Ho, Wo, mean=MEAN, std=STD):
    """fp64: ``F.interpolate(antialias=True)`` of each cropped image, normalised with the fp32 constants the
    pipeline uses, flipped -> [B, C, Ho, Wo]."""
    data = torch.as_tensor(data)
    C = data.shape[-1]
    m = torch.tensor(mean[:C], dtype=torch.float32).double().view(C, 1, 1)
    s = torch.tensor(std[:C], dtype=torch.float32).double().view(C, 1, 1)
    out = []
    for d in idx:
        top, left, h, w, flip = (int(v) for v in table[d])
        crop = data[d, top:top + h, left:left + w].permute(2, 0, 1).double().unsqueeze(0) / 255.0
        v = F.interpolate(crop, size=(Ho, Wo), mode="bilinear", antialias=True, align_corners=False)[0]
        v = (v - m) / s
        out.append(v.flip(-1) if flip else v)
    return torch.stack(out)


def write_arrays(root, n_train=64, n_val=16, side=40, classes=4):
    """The trainer's fixture: {train,val}_images.npy (uint8 [n, side, side, 3]) and _labels.npy under ``root``."""
    g = np.random.default_rng(0)
    os.makedirs(root, exist_ok=True)
    for split, n in (("train", n_train), ("val", n_val)):
        np.save(os.path.join(root, f"{split}_images.npy"), g.integers(0, 256, (n, side, side, 3), dtype=np.uint8))
        np.save(os.path.join(root, f"{split}_labels.npy"), g.integers(0, classes, n).astype(np.int64))
