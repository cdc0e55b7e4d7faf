"""Shapes, transforms and sources shared by tests/test_seg_aug_cpu.py and tests/test_seg_aug_gpu.py."""
import numpy as np
import torch

from deeplearning_mpi_amd.data import seg_affine

# (C, H, W, Ho, Wo): same size odd / even, a crop, a larger output
SHAPES = [(3, 17, 23, 17, 23), (1, 8, 12, 8, 12), (3, 17, 23, 9, 11), (2, 16, 16, 24, 20)]
# keyword arguments of seg_affine
TRANSFORMS = {
    "identity": {},
    "hflip": dict(hflip=True),
    "vflip": dict(vflip=True),
    "flips_shift": dict(hflip=True, vflip=True, tx=3, ty=-2),
    "rot90": dict(degrees=90),
    "zoom_rot": dict(scale=1.3, degrees=30, tx=1.7, ty=-2.2),
    "flip_shrink_rot": dict(hflip=True, scale=0.77, degrees=-17, tx=0.3, ty=4.1),
    "outside": dict(tx=100, ty=0),
}
# coordinates that land on .5 for some sizes: they pin the nearest rule (a tie rounds up)
TIES = {"half": dict(scale=0.5), "double": dict(scale=2), "half_shift": dict(tx=0.5, ty=0.5)}


def sources(N, C, H, W, mask_dtype=torch.float32, seed=0):
    """images fp32 [N, C, H, W] in [0, 1); masks [N, H, W]: class indices 0..4 in ``mask_dtype``."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    images = torch.rand(N, C, H, W, generator=g)
    masks = torch.randint(5, (N, H, W), generator=g).to(mask_dtype)
    return images, masks


def table_of(transforms, H, W, Ho, Wo):
    """int32 [len(transforms), 6]: row i the matrix of transforms[i] (a dict of seg_affine's keywords)."""
    return np.array([seg_affine(H, W, Ho, Wo, **t) for t in transforms], dtype=np.int32)
