"""ctypes binding of the C ABI declared in include/i2sdf.h (libi2sdf_hip.so, built in-tree by
i2sdf_amd/csrc/build.sh or __graft_entry__.build()).  No CPU fallback: a missing library or a failing call raises."""
from __future__ import annotations

import ctypes as C
import os

MAX_LAYERS = 12
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("I2SDF_LIB_PATH") or os.path.join(_HERE, "lib", "libi2sdf_hip.so")     # override: A/B of two builds on one box


class MlpDesc(C.Structure):
    _fields_ = [("n_lin", C.c_int32), ("hidden", C.c_int32), ("d_in", C.c_int32), ("in0", C.c_int32), ("d_out", C.c_int32),
                ("multires", C.c_int32), ("skip_layer", C.c_int32), ("reserved", C.c_int32),
                ("out_dim", C.c_int32 * MAX_LAYERS), ("in_dim", C.c_int32 * MAX_LAYERS),
                ("off_bias", C.c_int64 * MAX_LAYERS), ("off_g", C.c_int64 * MAX_LAYERS), ("off_v", C.c_int64 * MAX_LAYERS)]


class NetDesc(C.Structure):
    _fields_ = [("sdf", MlpDesc), ("rgb", MlpDesc), ("light", MlpDesc), ("off_beta", C.c_int64), ("n_params", C.c_int64),
                ("beta_min", C.c_float), ("scene_bounding_sphere", C.c_float)]


class TrainBuffers(C.Structure):
    _fields_ = [("M_sdf", C.c_int64), ("M_main", C.c_int64), ("Mp", C.c_int64)] + [(n, C.c_void_p) for n in (
        "pe", "hs", "abars", "gus", "gpbar", "gas", "ga_last4", "ones4", "fbar", "pev", "feat", "rs", "gar", "ga_last_rgb",
        "hl", "gal0", "gal_last")]


class SamplerCfg(C.Structure):
    _fields_ = [("near", C.c_float), ("eps", C.c_float), ("add_tiny", C.c_float), ("N_samples", C.c_int32), ("N_samples_eval", C.c_int32),
                ("N_samples_extra", C.c_int32), ("beta_iters", C.c_int32), ("max_total_iters", C.c_int32)]


# int allreduce(void* ctx, void* buf, int64_t n, int32_t dtype, int32_t op, void* stream)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p)


class Exchange(C.Structure):
    _fields_ = [("allreduce", EXCHANGE_FN), ("ctx", C.c_void_p)]


class TraceCfg(C.Structure):
    _fields_ = [("eps", C.c_float), ("step_scale", C.c_float), ("max_steps", C.c_int32), ("route", C.c_int32)]


class LossCfg(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("eikonal_w", "smooth_w", "mask_w", "depth_w", "normal_w", "angular_w", "bubble_w", "light_w")] + \
               [("smooth_on", C.c_int32), ("reserved", C.c_int32), ("exchange", C.POINTER(Exchange))]


XCHG_F32, XCHG_I32 = 0, 1
XCHG_SUM, XCHG_AVG, XCHG_MAX = 0, 1, 2
DP_GLOBAL_SAMPLER = 1
COMM_UNIQUE_ID_BYTES = 128


class RayTables(C.Structure):
    _fields_ = [("intrinsics", C.c_void_p), ("pose", C.c_void_p), ("pose_is_quat", C.c_int32), ("n_images", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("rgb", "depth", "normal", "mask", "light_mask", "depth_mask", "normal_mask")]


class RayBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("image_idx", "uv", "cam_loc", "dirs", "dnorm", "rgb", "depth", "normal", "mask", "light_mask",
                                          "depth_mask", "normal_mask", "n_bad")]


OPT_SDF_FWD_BF16X3 = 1
OPT_WGRAD_BF16X3 = 2
OPT_TRAIN_FWD_BF16X3 = 4
OPT_SDF_BWD_BF16X3 = 8
OPT_RGB_BF16X3 = 16
OPT_TAIL_OVERLAP = 32
OPT_BLOCKED_SAVES = 128
OPT_WGRAD_BF16X2 = 256
OPT_PARTS = 512
OPT_SAMPLER_BF16X2 = 1024
OPT_SAVES24 = 2048
MAX_PARTS = 4
GRID_ORDER_MESHGRID, GRID_ORDER_VOLUME = 0, 1
RGB_MODE_NERF, RGB_MODE_IDR = 0, 1    # I2SDF_RGB_MODE_*: i2sdf_net_desc.rgb.reserved, bits 0..7
RGB_ACTS = {"sigmoid": 0, "relu": 1, "softplus": 2}      # I2SDF_RGB_ACT_*: the same field, bits 8..15 (reserved = mode | act << 8)
RGB_EMBEDS = {"positional": 0, "spherical_harmonics": 1, "fourier": 2}      # I2SDF_RGB_EMBED_*: the same field, bits 24..27
RGB_EMBED_MAX_CHANNELS = 12      # I2SDF_RGB_EMBED_MAX_CHANNELS
RASTER_SMALL_MAX = 64            # I2SDF_RASTER_SMALL_MAX
TSDF_MAX_CELLS = 1 << 24         # I2SDF_TSDF_MAX_CELLS
IMAGE_STATS = 8                  # I2SDF_IMAGE_STATS
SSIM_TILE_X, SSIM_TILE_Y = 32, 16    # I2SDF_SSIM_TILE_X, I2SDF_SSIM_TILE_Y
BUBBLE_MAX_K = 4096              # I2SDF_BUBBLE_MAX_K
BUBBLE_WS_PASSES_OFFSET = 24     # I2SDF_BUBBLE_WS_PASSES_OFFSET
KMEANS_MAX_K = 256               # I2SDF_KMEANS_MAX_K
DBSCAN_NONFINITE, DBSCAN_CELLS = 1, 2    # I2SDF_DBSCAN_*: status bits
RAYCAST_BAD_RAY, RAYCAST_BAD_FACE = 1, 2    # I2SDF_RAYCAST_*: status bits
RAYCAST_CULL = {"none": 0, "back": 1}      # I2SDF_RAYCAST_CULL_*
BVH_MAX_FACES = 1 << 28          # I2SDF_BVH_MAX_FACES
CLOSEST_BAD_POINT, CLOSEST_BAD_FACE = 1, 2  # I2SDF_CLOSEST_*: status bits
# I2SDF_CLOSEST_FACE ... I2SDF_CLOSEST_VERT_C: the feature of the face the closest point lies on
CLOSEST_FEATURES = {"FACE": 0, "EDGE_AB": 1, "EDGE_BC": 2, "EDGE_CA": 3, "VERT_A": 4, "VERT_B": 5, "VERT_C": 6}
WINDING_BAD_POINT, WINDING_BAD_FACE = 1, 2  # I2SDF_WINDING_*: status bits
SIMPLIFY_CONTRACTIONS = {"quadric": 0, "average": 1}      # I2SDF_SIMPLIFY_QUADRIC / _AVERAGE
SIMPLIFY_BAD_FACE = 1            # I2SDF_SIMPLIFY_BAD_FACE: status bit
SIMPLIFY_DROP_REPEATED, SIMPLIFY_DROP_ZERO_AREA = 1, 2    # I2SDF_SIMPLIFY_DROP_*: flags of i2sdf_simplify_face_keys
# I2SDF_TOPO_*: indices into the counts of i2sdf_mesh_edge_stats
TOPO = {"EDGES": 0, "BOUNDARY": 1, "MANIFOLD": 2, "NONMANIFOLD": 3, "MISORIENTED": 4, "REPEATED_FACES": 5, "VERTICES": 6, "EULER": 7, "FACES": 8}
TOPO_COUNTS = 10                 # I2SDF_TOPO_COUNTS
TRACE_HIT, TRACE_MISS, TRACE_UNRESOLVED, TRACE_INSIDE = 1, 2, 3, 4      # I2SDF_TRACE_*: status of a traced ray
TRACE_ROUTES = {"auto": 0, "stepwise": 1, "fused": 2}                   # I2SDF_TRACE_AUTO / _STEPWISE / _FUSED
TRACE_MAX_STEPS = 1024           # I2SDF_TRACE_MAX_STEPS


class I2SDFError(RuntimeError):
    pass


_lib = None

# name -> (restype, argtypes).  Must list every symbol include/i2sdf.h declares (tests/test_cabi.py checks it).
_P, _I64, _I32, _F, _D = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_double
SIGNATURES = {
    "i2sdf_version": (C.c_int, []),
    "i2sdf_strerror": (C.c_char_p, [C.c_int]),
    "i2sdf_last_hip_error": (C.c_char_p, []),
    "i2sdf_plan_create": (C.c_int, [C.POINTER(NetDesc), C.POINTER(_P)]),
    "i2sdf_plan_destroy": (None, [_P]),
    "i2sdf_plan_set_option": (C.c_int, [_P, _I32, _I32]),
    "i2sdf_chain_begin": (C.c_int, [_P, _I64, _P]),
    "i2sdf_chain_fence": (C.c_int, [_P, _P]),
    "i2sdf_chain_end": (C.c_int, [_P, _P]),
    "i2sdf_blocked_points": (_I64, [_P, _I32, _I64, _I64, _I32]),
    "i2sdf_plan_pack_floats": (_I64, [_P]),
    "i2sdf_plan_wgrad_floats": (_I64, [_P]),
    "i2sdf_pack_weights": (C.c_int, [_P, _P, _P, _P]),
    "i2sdf_sdf_forward": (C.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P]),
    # plan, packed, points, cam, dirs, z, ldz, n_per_ray, n_ray_pts, M, Mp, sdf, feat, grad, hs, abars, pe_save, stream
    "i2sdf_sdf_forward_grad": (C.c_int, [_P] * 6 + [_I64, _I32, _I64, _I64, _I64] + [_P] * 7),
    # plan, B_host (3, c) fp32 in host memory, rows, cols
    "i2sdf_plan_set_view_embed": (C.c_int, [_P, _P, _I32, _I32]),
    # plan, packed, dirs, n_per_ray, feat, M, Mp, rgb, rs, pev_save, stream
    "i2sdf_rgb_forward": (C.c_int, [_P, _P, _P, _I32, _P, _I64, _I64, _P, _P, _P, _P]),
    # plan, packed, rgb, rgb_bar, rs, M, Mp, gar, ga_last, fbar, stream
    "i2sdf_rgb_backward": (C.c_int, [_P] * 5 + [_I64, _I64] + [_P] * 4),
    # plan, packed, points, cam, dirs, z, ldz, n_per_ray, normals, feat, M, Mp, rgb, rs, pev_save, stream
    "i2sdf_rgb_forward_idr": (C.c_int, [_P] * 6 + [_I64, _I32, _P, _P, _I64, _I64] + [_P] * 4),
    # plan, packed, rgb, rgb_bar, rs, M, Mp, gar, ga_last, fbar, nbar, accumulate, stream
    "i2sdf_rgb_backward_idr": (C.c_int, [_P] * 5 + [_I64, _I64] + [_P] * 4 + [_I32, _P]),
    # plan, packed, points, cam, dirs, z, ldz, n_per_ray, n_ray_pts, M, Mp, hs, abars, sbar, fbar, m_fbar, nbar, gus, gpbar, gas,
    # ga_last4, ones4, stream
    "i2sdf_sdf_backward": (C.c_int, [_P] * 6 + [_I64, _I32, _I64, _I64, _I64] + [_P] * 4 + [_I64] + [_P] * 7),
    "i2sdf_wgrad_chunk_points": (_I64, []),
    "i2sdf_weight_grads": (C.c_int, [_P, C.POINTER(TrainBuffers), _P, _P, _I64, _P, _P]),
    "i2sdf_comm_available": (_I32, []),
    "i2sdf_comm_unique_id": (C.c_int, [_P, _I64]),
    "i2sdf_comm_init_rank": (C.c_int, [_P, _I32, _I32, C.POINTER(_P)]),
    "i2sdf_comm_destroy": (None, [_P]),
    "i2sdf_comm_size": (_I32, [_P]),
    "i2sdf_comm_rank": (_I32, [_P]),
    "i2sdf_last_comm_error": (C.c_char_p, []),
    "i2sdf_allreduce_grads": (C.c_int, [_P, _I64, _P, _P]),
    "i2sdf_allreduce_max_i32": (C.c_int, [_P, _I64, _P, _P]),
    "i2sdf_broadcast": (C.c_int, [_P, _I64, _I32, _P, _P]),
    "i2sdf_comm_as_exchange": (C.c_int, [_P, C.POINTER(Exchange)]),
    "i2sdf_plan_set_exchange": (C.c_int, [_P, C.POINTER(Exchange), _I32]),
    "i2sdf_adam_step": (C.c_int, [_P, _P, _P, _P, _I64, _D, _D, _D, _D, _D, _I64, _D, _P]),
    "i2sdf_error_bound": (C.c_int, [_P, _P, _I64, _I32, _P, _I64, _P, _P, _P, _P]),
    "i2sdf_sampler_workspace_floats": (_I64, [_I64]),
    # plan, packed, params, cfg, cam, dirs, B, training, t_lin, u_more, u_final, ldu_final, extra_tab, strat_u, extra_idx, eik_idx,
    # force_iters, workspace, z_out, ldz, z_eik, iters_out, stream
    "i2sdf_sample_rays": (C.c_int, [_P, _P, _P, C.POINTER(SamplerCfg), _P, _P, _I64, _I32, _P, _P, _P, _I64, _P, _P, _P, _P, _I32, _P, _P,
                                    _I64, _P, _P, _P]),
    "i2sdf_render_image_workspace_floats": (_I64, [_P, C.POINTER(SamplerCfg), _I64]),
    # plan, packed, params, cfg, uv, pose, pose_is_quat, intrinsics, P, chunk, t_lin, u_more, u_final, extra_tab, workspace,
    # o_rgb, o_depth, o_wsum, o_normal, o_lmask, o_z, o_iters, stream
    "i2sdf_render_image": (C.c_int, [_P, _P, _P, C.POINTER(SamplerCfg), _P, _P, _I32, _P, _I64, _I64] + [_P] * 13),
    "i2sdf_sdf_grid_workspace_floats": (_I64, [_I64]),
    # plan, packed, x, y, z, nx, ny, nz, order, rot (host), trans (host), first, count, sdf_out, workspace, chunk_points, stream
    "i2sdf_sdf_grid": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _I64, _I64, _P, _P, _I64, _P]),
    "i2sdf_marching_cubes_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    # vol, nx, ny, nz, level, workspace, counts_out, stream
    "i2sdf_marching_cubes_count": (C.c_int, [_P, _I32, _I32, _I32, _F, _P, _P, _P]),
    # vol, nx, ny, nz, level, spacing (host), origin (host), workspace, verts, normals, faces, cap_v, cap_f, stream
    "i2sdf_marching_cubes_emit": (C.c_int, [_P, _I32, _I32, _I32, _F, _P, _P, _P, _P, _P, _P, _I64, _I64, _P]),
    "i2sdf_mesh_scan_workspace_bytes": (_I64, [_I64]),
    "i2sdf_mesh_status": (C.c_int, [_P, _P]),
    # faces, F, n_verts, keys, status, stream
    "i2sdf_mesh_edge_keys": (C.c_int, [_P, _I64, _I64, _P, _P, _P]),
    # sorted_keys, perm, F, labels, stream
    "i2sdf_mesh_face_components": (C.c_int, [_P, _P, _I64, _P, _P]),
    # verts, n_verts, faces, F, area, status, stream
    "i2sdf_mesh_face_areas": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P]),
    # x, n_x, order, n, cdf, workspace, stream
    "i2sdf_mesh_cumsum_f64": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P]),
    # sorted_labels, cdf, F, best, stream
    "i2sdf_mesh_largest_label": (C.c_int, [_P, _P, _I64, _P, _P]),
    # faces, mask, F, n_verts, fkeep, vflag, status, stream
    "i2sdf_mesh_compact_mark": (C.c_int, [_P, _P, _I64, _I64, _P, _P, _P, _P]),
    # verts, normals, n_verts, faces, F, fkeep, fscan, vflag, vscan, out_verts, out_normals, out_faces, cap_v, cap_f, stream
    "i2sdf_mesh_compact_gather": (C.c_int, [_P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _P]),
    # verts, n_verts, faces, F, cdf, u_face, u_bary, count, points, face_index, status, stream
    "i2sdf_mesh_sample_surface": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P]),
    # points, n, bounds, status, stream
    "i2sdf_points_bounds": (C.c_int, [_P, _I64, _P, _P, _P]),
    # points, n, bounds, voxel_size, keys, status, stream
    "i2sdf_points_voxel_keys": (C.c_int, [_P, _I64, _P, _D, _P, _P, _P]),
    # sorted_keys, n, heads, stream
    "i2sdf_points_voxel_heads": (C.c_int, [_P, _I64, _P, _P]),
    # points, n, sorted_keys, perm, head_scan, out_points, out_counts, cap_m, stream
    "i2sdf_points_voxel_mean": (C.c_int, [_P, _I64, _P, _P, _P, _P, _P, _I64, _P]),
    "i2sdf_points_grid_workspace_bytes": (_I64, [_I64]),
    # ref, n_ref, workspace, keys, status, stream
    "i2sdf_points_grid_keys": (C.c_int, [_P, _I64, _P, _P, _P, _P]),
    # ref, n_ref, sorted_keys, perm, workspace, sorted_ref, stream
    "i2sdf_points_grid_build": (C.c_int, [_P, _I64, _P, _P, _P, _P, _P]),
    # query, n_query, sorted_ref, n_ref, workspace, max_ring, dist, index, fallback_list, status, stream
    "i2sdf_points_nn_query": (C.c_int, [_P, _I64, _P, _I64, _P, _I32, _P, _P, _P, _P, _P]),
    # query, n_query, ref, n_ref, fallback_list, status, dist, index, stream
    "i2sdf_points_nn_fallback": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P, _P, _P]),
    "i2sdf_points_reduce_workspace_bytes": (_I64, [_I64]),
    # dist, n, threshold, workspace, out, stream
    "i2sdf_points_threshold_reduce": (C.c_int, [_P, _I64, _D, _P, _P, _P]),
    "i2sdf_raster_workspace_bytes": (_I64, [_I64, _I64, _I32]),
    # verts, n_verts, faces, F, w2c, n_cam, K4 (host), H, W, znear, zfar, cull, workspace, depth, counters, status, stream
    "i2sdf_raster_depth": (C.c_int, [_P, _I64, _P, _I64, _P, _I32, _P, _I32, _I32, _F, _F, _I32, _P, _P, _P, _P, _P]),
    "i2sdf_tsdf_table_cells": (_I64, [_P]),
    "i2sdf_tsdf_extract_workspace_bytes": (_I64, [_I64]),
    # depths, n_cam, H, W, c2w, K4 (host), voxel_length, unit_length, sdf_trunc, depth_trunc, stride, bounds, stream
    "i2sdf_tsdf_bounds": (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _F, _F, _F, _F, _I32, _P, _P]),
    # depths, n_cam, cam, H, W, c2w, K4, voxel_length, unit_length, sdf_trunc, depth_trunc, stride, grid6 (host), slot, n_units, stamp,
    # list, list_count, flag, stream
    "i2sdf_tsdf_mark": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _F, _F, _F, _F, _I32, _P, _P, _I64, _P, _P, _P, _P, _P]),
    # depths, n_cam, cam, H, W, w2c, K4, voxel_length, unit_length, sdf_trunc, depth_trunc, grid6, unit_cell, n_units, list, list_count,
    # tsdf, weight, stream
    "i2sdf_tsdf_integrate": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _F, _F, _F, _F, _P, _P, _I64, _P, _P, _P, _P, _P]),
    # grid6, slot, unit_cell, n_units, tsdf, weight, workspace, blocks, stream
    "i2sdf_tsdf_count": (C.c_int, [_P, _P, _P, _I64, _P, _P, _P, _P, _P]),
    # grid6, voxel_length, unit_length, slot, unit_cell, n_units, tsdf, weight, workspace, blocks_excl, verts, normals, faces, cap_v, cap_f, stream
    "i2sdf_tsdf_emit": (C.c_int, [_P, _F, _F, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _P]),
    "i2sdf_image_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    # pred, gt, depth, n_views, H, W, workspace, stats, stream
    "i2sdf_image_stats": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    # pred, gt, n_views, H, W, data_range, stats, workspace, ssim, map, stream
    "i2sdf_image_ssim": (C.c_int, [_P, _P, _I32, _I32, _I32, _F, _P, _P, _P, _P, _P]),
    # rgb, normal, depth, pose, stats, lut, n_views, H, W, rgb8, normal8, normal_cam, depth8, depth_rgb8, stream
    "i2sdf_image_frames": (C.c_int, [_P] * 6 + [_I32, _I32, _I32] + [_P] * 6),
    # src, dst, n, clamp01, stream
    "i2sdf_linear_to_srgb": (C.c_int, [_P, _P, _I64, _I32, _P]),
    # pred, target, channels, pixel_idx, first_pixel, n, pointlinks, n_links, pdf_max, pdf_prune, pdf, n_pdf, n_bad, stream
    "i2sdf_pdf_update": (C.c_int, [_P, _P, _I32, _P, _I64, _I64, _P, _I64, C.c_double, C.c_double, _P, _I64, _P, _P]),
    # seed, B, n_eval, n_samples, n_extra, max_iters, n_z, eik_radius, nbr_half_width, strat_u, cdf_u, extra_idx, eik_idx, eik_pts, nbr_off, stream
    "i2sdf_training_draws": (C.c_int, [C.c_uint64, _I64, _I32, _I32, _I32, _I32, _I32, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "i2sdf_bubble_sample_workspace_bytes": (_I64, [_I64]),
    # weights, n, pointcloud, k, seed, draw, workspace, idx, points, sample_count, status, stream
    "i2sdf_bubble_sample": (C.c_int, [_P, _I64, _P, _I64, C.c_uint64, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    # weights, n, seed, draw, keys_out, stream
    "i2sdf_bubble_keys": (C.c_int, [_P, _I64, C.c_uint64, C.c_uint32, _P, _P]),
    "i2sdf_depth_unproject_workspace_bytes": (_I64, [_I64, _I32, _I32]),
    # depth, n_img, H, W, lo, hi, workspace, depth_masks, n_points (host), stream
    "i2sdf_depth_unproject_count": (C.c_int, [_P, _I64, _I32, _I32, _F, _F, _P, _P, C.POINTER(_I64), _P]),
    # depth, intrinsics, pose, n_img, H, W, lo, hi, workspace, n_points, pointlinks, pixlinks, pointcloud, stream
    "i2sdf_depth_unproject_write": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _F, _F, _P, _I64, _P, _P, _P, _P]),
    # seed, bn, spp, samples, stream
    "i2sdf_shade_draws": (C.c_int, [C.c_uint64, _I64, _I32, _P, _P]),
    # surface_points, view_direction, normal, Kd, Ks, rough, samples, seed (host), bn, spp, direction, points, wi_mask, stream
    "i2sdf_shade_sample": (C.c_int, [_P] * 7 + [C.POINTER(C.c_uint64), _I64, _I32] + [_P] * 4),
    # view_direction, normal, Kd, Ks, rough, samples, seed (host), radiance, radiance_scale, bn, spp, colorDiffuse, colorSpec, stream
    "i2sdf_shade_reduce": (C.c_int, [_P] * 6 + [C.POINTER(C.c_uint64), _P, _P, _I64, _I32] + [_P] * 3),
    "i2sdf_shade_backward_workspace_bytes": (_I64, [_I64, _I32]),
    # view_direction, normal, Kd, Ks, rough, samples, seed (host), radiance, radiance_scale, g_colorDiffuse, g_colorSpec, g_direction,
    # g_points, bn, spp, workspace, gKd, gKs, grough, g_radiance, g_radiance_scale, stream
    "i2sdf_shade_backward": (C.c_int, [_P] * 6 + [C.POINTER(C.c_uint64)] + [_P] * 6 + [_I64, _I32] + [_P] * 7),
    "i2sdf_kmeans_workspace_bytes": (_I64, [_I64, _I64]),
    # points, n, k, seed, workspace, idx_out, centroids_out, stream
    "i2sdf_kmeans_pp": (C.c_int, [_P, _I64, _I64, C.c_uint64, _P, _P, _P, _P]),
    # points, n, k, centroids (in / out), max_iter, tol, workspace, labels, n_iter (device), stream
    "i2sdf_kmeans_fit": (C.c_int, [_P, _I64, _I64, _P, _I32, _D, _P, _P, _P, _P]),
    # points, n, centroids, k, labels, dist2, stream
    "i2sdf_kmeans_assign": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P]),
    "i2sdf_dbscan_workspace_bytes": (_I64, [_I64]),
    # points, n, eps, workspace, keys, status, stream
    "i2sdf_dbscan_cell_keys": (C.c_int, [_P, _I64, _D, _P, _P, _P, _P]),
    # points, n, eps, min_samples, sorted_keys, perm, workspace, labels, core, n_clusters, status, stream
    "i2sdf_dbscan_label": (C.c_int, [_P, _I64, _D, _I32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "i2sdf_trace_workspace_floats": (_I64, [_I64]),
    # plan, packed, cfg, cam, dirs, t_min, t_max, N, t_out, status_out, steps_out, f_trace, workspace, stream
    "i2sdf_trace_rays": (C.c_int, [_P, _P, C.POINTER(TraceCfg)] + [_P] * 4 + [_I64] + [_P] * 6),
    "i2sdf_bvh_bytes": (_I64, [_I64]),
    # verts, V, faces, F, bvh, keys, stream
    "i2sdf_bvh_keys": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P]),
    # verts, V, faces, F, sorted_keys, bvh, stream
    "i2sdf_bvh_build": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P]),
    # bvh, F, orig, dirs, t_min, t_max, n, cull, any_hit, t, face, bary, hit, status, stream
    "i2sdf_bvh_trace": (C.c_int, [_P, _I64] + [_P] * 4 + [_I64, _I32, _I32] + [_P] * 6),
    # verts, V, faces, F, orig, dirs, t_min, t_max, n, cull, any_hit, t, face, bary, hit, status, stream
    "i2sdf_mesh_trace_brute": (C.c_int, [_P, _I64, _P, _I64] + [_P] * 4 + [_I64, _I32, _I32] + [_P] * 6),
    # bvh, verts, V, faces, F, points, n, max_dist, vnormal, enormal, dist, point, face, bary, feature, sdist, status, stream
    "i2sdf_closest_bvh": (C.c_int, [_P, _P, _I64, _P, _I64, _P, _I64, C.c_float] + [_P] * 10),
    # verts, V, faces, F, points, n, max_dist, vnormal, enormal, dist, point, face, bary, feature, sdist, status, stream
    "i2sdf_closest_brute": (C.c_int, [_P, _I64, _P, _I64, _P, _I64, C.c_float] + [_P] * 10),
    # verts, V, faces, F, keys, status, stream
    "i2sdf_closest_normal_keys": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P]),
    # verts, V, faces, F, sorted_keys, perm, vnormal, enormal, stream
    "i2sdf_closest_normals": (C.c_int, [_P, _I64, _P, _I64, _P, _P, _P, _P, _P]),
    "i2sdf_winding_moments_bytes": (_I64, [_I64]),
    # bvh, F, moments, stream
    "i2sdf_winding_moments": (C.c_int, [_P, _I64, _P, _P]),
    # bvh, moments, F, points, n, beta, w_out, status, stream
    "i2sdf_winding_bvh": (C.c_int, [_P, _P, _I64, _P, _I64, C.c_float, _P, _P, _P]),
    # verts, V, faces, F, points, n, w_out, status, stream
    "i2sdf_winding_brute": (C.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _P, _P]),
    # sorted_keys, perm, head_scan, V, n_cells, vertex_cell, cell_start, stream
    "i2sdf_simplify_vertex_cells": (C.c_int, [_P, _P, _P, _I64, _I64, _P, _P, _P]),
    # faces, F, V, vertex_cell, n_cells, corner_keys, status, stream
    "i2sdf_simplify_corner_keys": (C.c_int, [_P, _I64, _I64, _P, _I64, _P, _P, _P]),
    # sorted_corner_keys, F, n_cells, corner_runs, stream
    "i2sdf_simplify_corner_runs": (C.c_int, [_P, _I64, _I64, _P, _P]),
    # verts, normals, V, faces, F, bounds, voxel_size, reg, contraction, sorted_keys, perm, cell_start, corner_perm, corner_runs, n_cells,
    # out_verts, out_normals, fallback, stream
    "i2sdf_simplify_cells": (C.c_int, [_P, _P, _I64, _P, _I64, _P, C.c_double, C.c_double, _I32] + [_P] * 5 + [_I64] + [_P] * 4),
    # verts, V, faces, F, vertex_map, n_map, flags, out_faces, key_hi, key_lo, status, stream
    "i2sdf_simplify_face_keys": (C.c_int, [_P, _I64, _P, _I64, _P, _I64, _I32] + [_P] * 5),
    # sorted_hi, sorted_lo, perm, n, keep, first, stream
    "i2sdf_simplify_run_heads": (C.c_int, [_P, _P, _P, _I64, _P, _P, _P]),
    # verts, V, key_hi, key_lo, stream
    "i2sdf_simplify_position_keys": (C.c_int, [_P, _I64, _P, _P, _P]),
    # faces, F, V, keys, vflag, counts, status, stream
    "i2sdf_mesh_edge_stats_keys": (C.c_int, [_P, _I64, _I64, _P, _P, _P, _P, _P]),
    # sorted_keys, F, counts, stream
    "i2sdf_mesh_edge_stats": (C.c_int, [_P, _I64, _P, _P]),
    "i2sdf_light_forward": (C.c_int, [_P, _P, _P, _I64, _I64, _P, _P, _P]),
    "i2sdf_light_backward": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _P, _P, _P]),
    "i2sdf_loss_scratch_floats": (_I64, []),
    "i2sdf_loss_forward_backward": (C.c_int, [C.POINTER(LossCfg), _I64, _I64] + [_P] * 27),
    "i2sdf_eikonal_outputs_forward": (C.c_int, [_P, _I64, _P, _P, _P]),
    "i2sdf_extra_points": (C.c_int, [_P, _P, _P, _P, _P, _I64, _P, _P]),
    "i2sdf_render_loss_scratch_floats": (_I64, [_I64]),
    # cfg, B, n, n_pc, M_main, M_sdf, n_eik | beta_param, beta_min, z, ldz, sdf, rgb_pts, grad_pts, dnorm, nsum_save | 8 outputs | 7 ground truth |
    # scratch, losses, loss_value | 8 seeds | sdf_bar, rgb_bar, grad_bar, normal_term, lmask_bar, beta_grad, stream
    "i2sdf_render_loss_backward": (C.c_int, [C.POINTER(LossCfg), _I64, _I32, _I64, _I64, _I64, _I64, _P, C.c_float, _P, _I64] + [_P] * 5 + [_P] * 8 + [_P] * 7 +
                                   [_P] * 3 + [_P] * 8 + [_P, _P, _P, _I32, _P, _P, _P]),
    "i2sdf_scale_seeds": (C.c_int, [_P, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P]),
    "i2sdf_backward_seeds": (C.c_int, [_P, _I64, _P, _P, _I64, _I64, _P, _I64, _P, _I64, C.c_int32, _P]),
    "i2sdf_eikonal_outputs_backward": (C.c_int, [_P, _P, _P, _I64, _P, _P]),
    "i2sdf_ray_setup": (C.c_int, [_P, _P, _P, _I64, _I32, _P, _P, _P, _P]),
    "i2sdf_ray_setup_ex": (C.c_int, [_P, _P, _I32, _P, _I64, _I32, _P, _P, _P, _P]),
    "i2sdf_ray_batch": (C.c_int, [C.POINTER(RayTables), _P, _I64, C.POINTER(RayBatch), _P]),
    "i2sdf_sphere_intersections": (C.c_int, [_P, _P, _I64, _F, _P, _P, _P]),
    "i2sdf_composite_forward": (C.c_int, [_P, _F, _P, _I64, _P, _P, _P, _P, _P, _I64, _I32] + [_P] * 8),
    "i2sdf_composite_forward_eik": (C.c_int, [_P, _F, _P, _I64, _P, _P, _P, _P, _P, _I64, _I32] + [_P] * 11),
    "i2sdf_composite_backward": (C.c_int, [_P, _F, _P, _I64] + [_P] * 5 + [_I64, _I32] + [_P] * 12),
}


def load():
    """Load the HIP library or raise -- there is deliberately no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so.7; it must be in the process before our library so that both bind to the
    # SAME HIP runtime instance (streams and device pointers are shared between them).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise I2SDFError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc: int, what: str = "", reason: bool = False):
    """reason: the entry point leaves the reason of an I2SDF_EINVAL where i2sdf_last_hip_error() finds it"""
    if rc != 0:
        lib = load()
        msg = lib.i2sdf_strerror(rc).decode()
        # (plan creation leaves the reason of a refused shape there; the view embedder's entry points the reason of their refusals)
        if rc == -2 or (rc == -1 and (reason or what in ("i2sdf_plan_create", "i2sdf_plan_set_view_embed"))):
            msg += ": " + lib.i2sdf_last_hip_error().decode()
        if rc == -5:
            msg += ": " + lib.i2sdf_last_comm_error().decode()
        raise I2SDFError(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "C ABI needs contiguous tensors"
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
