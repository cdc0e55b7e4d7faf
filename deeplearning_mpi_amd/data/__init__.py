from .datasets import (CIFAR10, CarvanaDataset, CifarTransform, SegmentationDataset,  # noqa: F401
                       SyntheticImages, SyntheticMasks, device_batch)
from .sampler import DistributedSampler  # noqa: F401
from .device import (DeviceBatches, DeviceCachedDataset, DeviceImageDataset, DeviceSegDataset,  # noqa: F401
                     image_batch_reference)
from .mix import MixConfig, MixParams, draw_mix, mix_batch_, mix_reference  # noqa: F401
from .seg_aug import SegAugConfig, draw_seg_aug, draw_seg_params, seg_affine, seg_aug_reference  # noqa: F401
from .rrc import RrcConfig, center_box, draw_rrc, rrc_reference, rrc_taps, rrc_weights  # noqa: F401
