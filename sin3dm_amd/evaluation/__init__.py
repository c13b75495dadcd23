"""Geometry evaluation on the device: LP-IoU, LP-F-score and pairwise-IoU diversity (the reference's evaluation/patch_utils.py) and
SSFID (evaluation/ssfid.py)."""
from .patch_utils import (Patches, eval_div, eval_lp, extract_valid_patches, load_sdfgrid2vox, load_voxgrid, lp_maxima, lp_metrics,
                          pack_patches, pairwise_counts, pairwise_iou_dist, patch_validity, pool_occupancy, pooled_shape,
                          shuffled_choice)
from .ssfid import VoxelClassifier, eval_ssfid, frechet_distance, load_classifier_weights, ssfid_values

__all__ = ["Patches", "eval_div", "eval_lp", "extract_valid_patches", "load_sdfgrid2vox", "load_voxgrid", "lp_maxima", "lp_metrics",
           "pack_patches", "pairwise_counts", "pairwise_iou_dist", "patch_validity", "pool_occupancy", "pooled_shape", "shuffled_choice",
           "VoxelClassifier", "eval_ssfid", "frechet_distance", "load_classifier_weights", "ssfid_values"]
