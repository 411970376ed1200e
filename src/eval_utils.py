"""src/eval_utils.py of the reference: the metrics (its IOU / IOU_simple / preprocess helpers are file-format glue
and are not provided)."""
from parsenet_codebase_amd.fitting import to_one_hot  # noqa: F401
from parsenet_codebase_amd.metrics import (iou_segmentation, matching_iou, mean_IOU_one_sample,  # noqa: F401
                                           p_coverage, relaxed_iou, separate_losses)
