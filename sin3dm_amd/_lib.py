"""ctypes binding of libsin3dm_hip.so (C ABI: include/sin3dm_hip.h).

There is no CPU fallback: if the HIP library is missing or no MI355X is visible, every compute
entry point raises.  torch is used by the callers only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsin3dm_hip.so")

c_fp = C.POINTER(C.c_float)
c_i64p = C.POINTER(C.c_int64)

ABI_VERSION = 13
TAB_ROWS = ("sqrt_recip", "sqrt_recipm1", "coef1", "coef2", "logvar", "acp", "acp_prev")
KTAB_ROWS = ("sqrt_acp_prev", "sqrt_1m_acp_prev", "sqrt_1m_beta", "sqrt_beta")     # s3d_known_region.tables (S3D_KTAB_*)
MTAB_ROWS = ("cx", "c0", "c1", "cn")                                                # s3d_multistep.tables (S3D_MTAB_*)
STEP_DDPM, STEP_DDIM, STEP_MEAN_ONLY = 0, 1, 2
CARRY_OUT, CARRY_IN = 1, 2               # s3d_unet_step_film_carry flags (include/sin3dm_hip.h)
MEAN_START_X, MEAN_EPSILON = 0, 1
ERR_INVALID, ERR_MISSING, ERR_HIP, ERR_UNSUPPORTED, ERR_INTERNAL = -1, -2, -3, -4, -5
MAX_LANES = 16
MESHSDF_MAX_PAIRS = 1 << 27           # S3D_MESHSDF_MAX_PAIRS (include/sin3dm_hip.h): 1.5 GiB of (cell, triangle) pairs
MCS_MAX_BRICKS, MCS_MAX_SAMPLES = 1 << 27, 1 << 30      # S3D_MCS_MAX_BRICKS / S3D_MCS_MAX_SAMPLES
RENDER_MAX_PAIRS = 1 << 27           # S3D_RENDER_MAX_PAIRS: 1 GiB of (tile, triangle) pairs
RENDER_TILE, RENDER_SUBPIXEL, RENDER_MAX_COORD, RENDER_MAX_GRID = 16, 256, 1 << 20, 4096
IMGFEAT_INCEPTION, IMGFEAT_ALEXNET = 0, 1          # S3D_IMGFEAT_*
RENDER_AMBIENT, RENDER_DIFFUSE = 0.35, 0.65                    # S3D_RENDER_AMBIENT / S3D_RENDER_DIFFUSE
RENDER_MAX_LIGHTS, RENDER_PBR_MAX_MATERIALS, RENDER_MIN_ROUGHNESS = 4, 16, 0.089      # S3D_RENDER_MAX_LIGHTS / _PBR_MAX_MATERIALS / _MIN_ROUGHNESS
RENDER_RIG_INTENSITY, RENDER_PBR_AMBIENT = 0.5, 0.1            # S3D_RENDER_RIG_INTENSITY / S3D_RENDER_PBR_AMBIENT
RENDER_PASSES = ("shaded", "albedo", "metallic", "roughness", "normal", "geo")         # S3D_RENDER_PASS_*: the index is the value


class UNetCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("model_channels", C.c_int32), ("out_channels", C.c_int32),
                ("num_res_blocks", C.c_int32), ("n_levels", C.c_int32), ("channel_mult", C.c_int32 * 8),
                ("use_scale_shift_norm", C.c_int32), ("is_rollout", C.c_int32)]


class SamplerArgs(C.Structure):
    _fields_ = [("mode", C.c_int32), ("mean_type", C.c_int32), ("clip_denoised", C.c_int32),
                ("is_mask_t0", C.c_int32), ("eta", C.c_float), ("T", C.c_int32), ("batch", C.c_int64),
                ("per_sample", C.c_int64), ("model_out", C.c_void_p), ("x", C.c_void_p), ("noise", C.c_void_p),
                ("t", C.c_void_p), ("tables", C.c_void_p), ("y0", C.c_void_p), ("mask", C.c_void_p),
                ("sample", C.c_void_p), ("pred_xstart", C.c_void_p), ("mean", C.c_void_p)]


class KnownRegionArgs(C.Structure):
    """s3d_known_region: the known-region blend of a step (include/sin3dm_hip.h)."""
    _fields_ = [("y0", C.c_void_p), ("mask", C.c_void_p), ("noise", C.c_void_p), ("tables", C.c_void_p)]


class MultistepArgs(C.Structure):
    """s3d_multistep: the DPM-Solver++ multistep update of a step (include/sin3dm_hip.h)."""
    _fields_ = [("x0_prev", C.c_void_p), ("tables", C.c_void_p), ("order", C.c_int32)]


PROF_CLASSES = 4


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * PROF_CLASSES), ("flops", C.c_double * PROF_CLASSES), ("launches", C.c_int64 * PROF_CLASSES),
                ("forwards", C.c_int64), ("mfma_flops", C.c_double * PROF_CLASSES)]


class AeLossCfg(C.Structure):
    _fields_ = [("sdf_loss", C.c_int32), ("tex_loss", C.c_int32), ("sdf_threshold", C.c_float),
                ("tex_threshold_ratio", C.c_float), ("tex_weight", C.c_float)]


class DecoderCfg(C.Structure):
    _fields_ = [("geo_feat_channels", C.c_int32), ("tex_feat_channels", C.c_int32), ("feat_channel_up", C.c_int32),
                ("mlp_hidden_channels", C.c_int32), ("mlp_hidden_layers", C.c_int32), ("tex_channels", C.c_int32)]


# name -> (restype, argtypes); every symbol include/sin3dm_hip.h declares
SIGNATURES = {
    "s3d_abi_version": (C.c_int, []),
    "s3d_last_error": (C.c_char_p, []),
    "s3d_device_count": (C.c_int, []),
    "s3d_set_option": (C.c_int, [C.c_char_p, C.c_char_p]),
    "s3d_get_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "s3d_set_riders": (C.c_int, [C.c_int]),
    "s3d_unet_create": (C.c_int, [C.POINTER(UNetCfg), C.POINTER(C.c_void_p)]),
    "s3d_unet_destroy": (None, [C.c_void_p]),
    "s3d_unet_num_params": (C.c_int, [C.c_void_p]),
    "s3d_unet_param_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), c_i64p, C.POINTER(C.c_int)]),
    "s3d_unet_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64p, C.c_int]),
    "s3d_unet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p]),
    "s3d_unet_film_width": (C.c_int, [C.c_void_p]),
    "s3d_unet_film": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_unet_select_lane": (C.c_int, [C.c_void_p, C.c_int]),
    "s3d_unet_current_lane": (C.c_int, [C.c_void_p]),
    "s3d_unet_forward_film": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "s3d_unet_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "s3d_unet_profile_classes": (C.c_int, [C.c_void_p, C.c_int]),
    "s3d_unet_profile_read": (C.c_int, [C.c_void_p, C.POINTER(Profile)]),
    "s3d_unet_profile_kernel": (C.c_char_p, [C.c_void_p, C.c_int]),
    "s3d_sampler_step": (C.c_int, [C.POINTER(SamplerArgs), C.c_void_p]),
    "s3d_unet_step_film": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(SamplerArgs), C.c_void_p, C.c_void_p]),
    "s3d_unet_step_film_carry": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(SamplerArgs), C.c_void_p, C.c_void_p, C.c_int]),
    "s3d_sampler_step_known": (C.c_int, [C.POINTER(SamplerArgs), C.POINTER(KnownRegionArgs), C.c_void_p]),
    "s3d_unet_step_film_known": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(SamplerArgs), C.POINTER(KnownRegionArgs), C.c_void_p, C.c_void_p, C.c_int]),
    "s3d_sampler_step_multistep": (C.c_int, [C.POINTER(SamplerArgs), C.POINTER(MultistepArgs), C.POINTER(KnownRegionArgs), C.c_void_p]),
    "s3d_unet_step_film_multistep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(SamplerArgs), C.POINTER(MultistepArgs), C.c_void_p, C.c_void_p, C.c_int]),
    "s3d_sampler_renoise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                      C.c_void_p]),
    "s3d_op_triplane_conv": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p), C.c_void_p]),
    "s3d_op_triplane_norm_silu": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.c_void_p]),
    "s3d_op_triplane_resample": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                           C.POINTER(C.c_int), C.c_int, C.c_void_p]),
    "s3d_op_timestep_embed": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_op_triplane_resblock": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "s3d_decoder_create": (C.c_int, [C.POINTER(DecoderCfg), C.POINTER(C.c_void_p)]),
    "s3d_decoder_create_variant": (C.c_int, [C.POINTER(DecoderCfg), C.c_int32, C.POINTER(C.c_void_p)]),
    "s3d_decoder_out_channels": (C.c_int, [C.c_void_p]),
    "s3d_decoder_plane_features": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_decoder_destroy": (None, [C.c_void_p]),
    "s3d_decoder_num_params": (C.c_int, [C.c_void_p]),
    "s3d_decoder_param_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), c_i64p, C.POINTER(C.c_int)]),
    "s3d_decoder_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64p, C.c_int]),
    "s3d_decoder_prepare_triplane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.c_int, C.c_void_p]),
    "s3d_decoder_decode_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, c_fp, C.c_int, C.c_void_p,
                                            C.c_void_p]),
    "s3d_decoder_sdf_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, c_fp, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_decoder_grid_dims": (C.c_int, [c_fp, C.c_int, C.POINTER(C.c_int)]),
    "s3d_decoder_decode_grid": (C.c_int, [C.c_void_p, C.c_int, c_fp, C.c_void_p, C.c_void_p]),
    # iso-surface extraction
    "s3d_mc_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "s3d_mc_destroy": (None, [C.c_void_p]),
    "s3d_mc_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                               c_i64p, c_i64p, C.c_void_p]),
    "s3d_mc_extract": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_mesh_components": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    # narrow-band iso-surface extraction
    "s3d_mcs_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "s3d_mcs_destroy": (None, [C.c_void_p]),
    "s3d_mcs_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int)]),
    "s3d_mcs_seed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_i64p, c_i64p, C.c_void_p]),
    "s3d_mcs_pending": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_mcs_grow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_i64p, c_i64p, C.c_void_p]),
    "s3d_mcs_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64p, c_i64p, C.c_void_p]),
    "s3d_mcs_extract": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_mcs_occupancy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # textured mesh export: decimation, atlas texel positions, texture finishing
    "s3d_mesh_cluster_keys": (C.c_int, [C.c_void_p, C.c_int64, c_fp, C.c_float, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    "s3d_mesh_cluster_means": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "s3d_mesh_remap_faces": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_tex_face_corner0": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "s3d_tex_texel_positions": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_tex_quantize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_tex_dilate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # the field's normals as a tangent-space map on the atlas
    "s3d_tex_normal_texels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_tex_dilate_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # quadric-error decimation: quadrics, edge cost and target, edge validity, independent set, apply, face remap
    "s3d_mesh_qem_quadrics": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_mesh_qem_edge_cost": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "s3d_mesh_qem_edge_valid": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "s3d_mesh_qem_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_mesh_qem_apply": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_mesh_qem_remap_faces": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    # mesh to training data: band-limited closest point, winding number, surface samples, texel colours
    "s3d_meshsdf_bin_count": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, c_fp, C.c_float, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    "s3d_meshsdf_bin_fill": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, c_fp, C.c_float, C.POINTER(C.c_int), C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_meshsdf_closest": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, c_fp, C.c_float, C.POINTER(C.c_int),
                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_meshsdf_winding": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "s3d_meshsdf_face_areas": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "s3d_meshsdf_sample_surface": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "s3d_meshsdf_texture": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "s3d_meshsdf_texture_pbr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    # geometry evaluation: occupancy pooling, patch validity and packing, LP maxima, pairwise counts
    "s3d_eval_pool_or": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    "s3d_eval_patch_counts": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "s3d_eval_patch_valid": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_eval_pack_patches": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "s3d_eval_lp_max": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "s3d_eval_pack_volumes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "s3d_eval_pairwise_counts": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    # SSFID: classifier features, their mean and covariance
    "s3d_ssfid_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "s3d_ssfid_destroy": (None, [C.c_void_p]),
    "s3d_ssfid_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64p, C.c_int]),
    "s3d_ssfid_out_dims": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "s3d_ssfid_features": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_ssfid_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "s3d_ssfid_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    # image features of the renders: Inception stem statistics (SIFID), AlexNet pair distances (LPIPS)
    "s3d_imgfeat_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "s3d_imgfeat_destroy": (None, [C.c_void_p]),
    "s3d_imgfeat_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64p, C.c_int]),
    "s3d_imgfeat_out_dims": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "s3d_imgfeat_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                       C.c_void_p]),
    "s3d_imgfeat_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_imgfeat_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_imgfeat_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "s3d_imgfeat_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    # multi-view renders: project, bin, raster, shade
    "s3d_render_project": (C.c_int, [C.c_void_p, C.c_int64, c_fp, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_render_bin_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "s3d_render_bin_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_render_raster": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_render_shade": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   c_fp, c_fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_void_p]),
    # PBR renders: vertex normals, face tangents, the shade kernel with the GGX light model and the material passes
    "s3d_pbr_vertex_normals": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_pbr_face_tangents": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_pbr_shade": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       c_fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, c_i64p, c_fp, c_fp, c_fp, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    # ray queries against a mesh, the shadow mask of a view, the PBR shade kernel with the mask
    "s3d_mesh_ray_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_int64, c_fp, C.c_float,
                                        C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_pbr_shadow_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, c_fp,
                                         c_fp, C.c_int, C.c_float, C.c_void_p, c_fp, C.c_float, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p]),
    "s3d_pbr_shade_lit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    c_fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_void_p, c_i64p, c_fp, c_fp, c_fp, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # torch's CPU noise stream on the device
    "s3d_rng_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "s3d_rng_destroy": (None, [C.c_void_p]),
    "s3d_rng_set_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_void_p]),
    "s3d_rng_get_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.c_void_p]),
    "s3d_rng_reserve": (C.c_int, [C.c_void_p, C.c_int64]),
    "s3d_rng_randn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "s3d_rng_rand": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    # auto-encoder training tier
    "s3d_ae_create": (C.c_int, [C.POINTER(DecoderCfg), C.POINTER(C.c_void_p)]),
    "s3d_ae_create_variant": (C.c_int, [C.POINTER(DecoderCfg), C.c_int32, C.POINTER(C.c_void_p)]),
    "s3d_ae_create_pbr": (C.c_int, [C.POINTER(DecoderCfg), C.POINTER(C.c_void_p)]),
    "s3d_ae_out_channels": (C.c_int, [C.c_void_p]),
    "s3d_ae_destroy": (None, [C.c_void_p]),
    "s3d_ae_num_params": (C.c_int, [C.c_void_p]),
    "s3d_ae_param_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), c_i64p, C.POINTER(C.c_int), c_i64p]),
    "s3d_ae_param_numel": (C.c_int64, [C.c_void_p, c_i64p]),
    "s3d_ae_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "s3d_ae_repack": (C.c_int, [C.c_void_p, C.c_void_p]),
    "s3d_ae_set_volume": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "s3d_ae_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_ae_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, c_fp, C.c_void_p, C.c_void_p]),
    "s3d_ae_loss_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, c_fp, C.POINTER(AeLossCfg),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_ae_loss_grads_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, c_fp, C.POINTER(AeLossCfg),
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # training tier
    "s3d_unet_param_numel": (C.c_int64, [C.c_void_p]),
    "s3d_unet_param_offset": (C.c_int, [C.c_void_p, C.c_int, c_i64p]),
    "s3d_unet_train_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "s3d_unet_repack": (C.c_int, [C.c_void_p, C.c_void_p]),
    "s3d_unet_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "s3d_unet_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s3d_unet_backward_marked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int]),
    "s3d_train_q_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                     C.c_void_p, C.c_void_p]),
    "s3d_train_mse_terms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "s3d_train_mse_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "s3d_train_adamw_ema": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), c_fp, C.c_int,
                                      C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                      C.c_void_p]),
}

_lib = None


class Sin3DMHipError(RuntimeError):
    pass


def load():
    """dlopen the HIP library (no GPU needed just to load and inspect symbols)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            f"`make -C sin3dm_amd/csrc`. sin3dm_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = ABI drift, fail loudly
        fn.restype = res
        fn.argtypes = args
    v = lib.s3d_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"libsin3dm_hip.so ABI {v} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def last_error():
    return (load().s3d_last_error() or b"").decode(errors="replace")


def check(rc):
    """Map a status code to the exception type the reference would raise for the same mistake."""
    if rc == 0:
        return
    msg = last_error()
    if rc == ERR_INVALID:
        raise AssertionError(msg)
    if rc == ERR_MISSING:
        raise RuntimeError("Error(s) in loading state_dict: " + msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise Sin3DMHipError(msg)


def require_gpu(t=None):
    """The product path runs on MI355X only."""
    import torch
    if t is not None and not t.is_cuda:
        raise Sin3DMHipError("sin3dm_amd runs on an MI355X: tensor is on %s and there is no CPU fallback" % t.device)
    if not torch.cuda.is_available():
        raise Sin3DMHipError("sin3dm_amd needs a visible MI355X (torch.cuda.is_available() is False); "
                             "there is no CPU fallback")


def set_option(name, value):
    """Select a kernel form process-wide (include/sin3dm_hip.h: s3d_set_option); value None = the library's own choice."""
    check(load().s3d_set_option(str(name).encode(), None if value is None else str(value).encode()))


def get_option(name):
    v = C.c_int(0)
    check(load().s3d_get_option(str(name).encode(), C.byref(v)))
    return None if v.value == -1 else v.value


def set_riders(on):
    """Riders of the inference forward on (the default) or off (include/sin3dm_hip.h: s3d_set_riders); bit-identical."""
    check(load().s3d_set_riders(1 if on else 0))


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def ptr3(ts):
    return (C.c_void_p * 3)(*[C.c_void_p(t.data_ptr()) for t in ts])


def read_layout(n, info):
    """[(name, offset, numel, shape)] of a handle's n flat parameters; info(i, name, shape, ndim, offset) fills ctypes references for entry i
    (the handle's param_info, and its param_offset where that is a call of its own)."""
    layout = []
    for i in range(n):
        name, shape, nd, off = C.c_char_p(), (C.c_int64 * 5)(), C.c_int(), C.c_int64()
        info(i, C.byref(name), shape, C.byref(nd), C.byref(off))
        shp = tuple(shape[k] for k in range(nd.value))
        layout.append((name.value.decode(), off.value, math.prod(shp), shp))
    return layout
