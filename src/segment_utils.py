"""The hot-path part of src/segment_utils.py of the reference."""
from parsenet_codebase_amd.fitting import SIOU_matched_segments, relaxed_iou_fast, to_one_hot  # noqa: F401
from parsenet_codebase_amd.metrics import (SIOU, cluster_prob, cluster_prob_mutual,  # noqa: F401
                                           continuous_labels, coverage_metrics,
                                           dot_product_from_cluster_centers, iou_segmentation,
                                           matching_iou, mean_IOU_one_sample, primitive_type_segment,
                                           primitive_type_segment_torch, relaxed_iou)
from parsenet_codebase_amd.surface import sample_from_collection_of_mesh  # noqa: F401,E402
