from .act import Act, pad8  # noqa: F401
from .backend import NativeBackend, RefBackend, make_backend  # noqa: F401
from .losses import (BCEBoundaryLoss, BCEDiceLoss, BCELovaszLoss, BCEWithLogitsLoss, BoundaryLoss,  # noqa: F401
                     CEBoundaryLoss, CEDiceLoss, CELovaszLoss, CrossEntropyLoss, DiceLoss, LovaszHingeLoss,
                     LovaszSoftmaxLoss, OHEMBCEWithLogitsLoss, OHEMCrossEntropyLoss, backward, bce_boundary_loss,
                     bce_dice_loss, bce_lovasz_loss, bce_with_logits, boundary_loss, ce_boundary_loss, ce_dice_loss,
                     ce_lovasz_loss, cross_entropy, dice_loss, dice_multiclass, dice_per_sample, edt_squared,
                     lovasz_hinge, lovasz_softmax, mean_iou, ohem_bce_with_logits, ohem_cross_entropy, seg_counts,
                     signed_distance_map, surface_distances, top1_correct)
from ..data.mix import mix_batch_  # noqa: F401,E402  (the in-place mixup / CutMix kernel of data.hip)
