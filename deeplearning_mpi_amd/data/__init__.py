from .datasets import (CIFAR10, CarvanaDataset, CifarTransform, SegmentationDataset,  # noqa: F401
                       SyntheticImages, SyntheticMasks, device_batch)
from .sampler import DistributedSampler  # noqa: F401
from .device import DeviceBatches, DeviceCachedDataset, DeviceImageDataset, image_batch_reference  # noqa: F401
from .mix import MixConfig, MixParams, draw_mix, mix_batch_, mix_reference  # noqa: F401
