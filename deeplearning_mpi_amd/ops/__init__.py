from .act import Act, pad8  # noqa: F401
from .backend import NativeBackend, RefBackend, make_backend  # noqa: F401
from .losses import (BCEDiceLoss, BCEWithLogitsLoss, CEDiceLoss, CrossEntropyLoss, DiceLoss, backward,  # noqa: F401
                     bce_dice_loss, bce_with_logits, ce_dice_loss, cross_entropy, dice_loss, dice_multiclass,
                     dice_per_sample, mean_iou, seg_counts, top1_correct)
from ..data.mix import mix_batch_  # noqa: F401,E402  (the in-place mixup / CutMix kernel of data.hip)
