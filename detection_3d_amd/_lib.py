"""ctypes binding of libd3d_hip.so (include/d3d_hip.h).  There is NO CPU fallback: if the HIP
library is missing or fails to load, importing an op raises."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("D3D_LIB_PATH") or os.path.join(_HERE, "lib", "libd3d_hip.so")   # (the override: A/B runs of library builds)

_lib = None

c_int_p = ctypes.POINTER(ctypes.c_int)
c_float_p = ctypes.POINTER(ctypes.c_float)
vp = ctypes.c_void_p


class BnPrologue(ctypes.Structure):
    """d3d_bn_prologue (include/d3d_hip.h): device pointers of the producer's BatchNorm."""
    _fields_ = [("mean", vp), ("invstd", vp), ("weight", vp), ("bias", vp), ("leakiness", ctypes.c_float),
                ("out_stats", vp), ("out_stats_cap", ctypes.c_int), ("out_stats_rows", ctypes.POINTER(ctypes.c_int))]


bn_p = ctypes.POINTER(BnPrologue)


class ConvDesc(ctypes.Structure):
    """d3d_conv_desc (include/d3d_hip.h): one member of a grouped convolution call."""
    _fields_ = [("kind", ctypes.c_int), ("in_size", ctypes.c_int * 3), ("out_size", ctypes.c_int * 3),
                ("filter", ctypes.c_int * 3), ("stride", ctypes.c_int * 3), ("input", vp), ("cin", ctypes.c_int),
                ("packed_w", vp), ("cout", ctypes.c_int), ("residual", vp), ("out", vp), ("dtype", ctypes.c_int),
                ("macs_host", ctypes.POINTER(ctypes.c_double)), ("bn_host", bn_p), ("time_start", vp), ("time_stop", vp),
                ("form", c_int_p)]


class DepthFramesDesc(ctypes.Structure):
    """d3d_depth_frames (include/d3d_hip.h): a batch of posed depth frames, device pointers."""
    _fields_ = [("depth", vp), ("depth_is_u16", ctypes.c_int), ("color", vp), ("color_is_u8", ctypes.c_int),
                ("intrinsics", vp), ("extrinsics", vp), ("frames", ctypes.c_int), ("height", ctypes.c_int),
                ("width", ctypes.c_int), ("depth_scale", ctypes.c_double)]


class TsdfVolumeDesc(ctypes.Structure):
    """d3d_tsdf_volume (include/d3d_hip.h): a TSDF block volume, device pointers (origin: host values)."""
    _fields_ = [("voxel", ctypes.c_double), ("trunc", ctypes.c_double), ("origin", ctypes.c_double * 3), ("table", vp),
                ("table_slots", ctypes.c_int), ("block_coords", vp), ("max_blocks", ctypes.c_int),
                ("n_blocks", ctypes.c_int), ("state", vp), ("order", vp), ("tsdf", vp), ("weight", vp),
                ("color_state", vp), ("color_weight", vp)]


class TriangleMeshDesc(ctypes.Structure):
    """d3d_triangle_mesh (include/d3d_hip.h): a triangle mesh, device pointers."""
    _fields_ = [("vertices", vp), ("n_vertices", ctypes.c_int), ("triangles", vp), ("n_triangles", ctypes.c_int),
                ("vertex_color", vp), ("color_is_u8", ctypes.c_int)]


class AugmentParams(ctypes.Structure):
    """d3d_augment_params (include/d3d_hip.h): one scene's augmentation, host memory."""
    _fields_ = [("m", ctypes.c_double * 9), ("nrm", ctypes.c_double * 9), ("color", ctypes.c_double * 3),
                ("u1", ctypes.c_double * 3), ("u2", ctypes.c_double * 3), ("origin_offset", ctypes.c_int),
                ("color_col", ctypes.c_int), ("normal_col", ctypes.c_int), ("reserved", ctypes.c_int)]


class GlobalAlignDetails(ctypes.Structure):
    """d3d_global_align_details (include/d3d_hip.h): device buffers for the tables of a call, each NULL or filled."""
    _fields_ = [("hist", vp), ("cells", vp), ("cell_count", vp), ("target_bits", vp), ("corr", vp), ("peak_value", vp),
                ("peak_shift", vp), ("scores", vp)]


aug_p = ctypes.POINTER(AugmentParams)
frames_p = ctypes.POINTER(DepthFramesDesc)
volume_p = ctypes.POINTER(TsdfVolumeDesc)
mesh_p = ctypes.POINTER(TriangleMeshDesc)
c_double_p = ctypes.POINTER(ctypes.c_double)
c_int64_p = ctypes.POINTER(ctypes.c_int64)

_SIGS = {
    "d3d_last_error": (ctypes.c_char_p, []),
    "d3d_abi_version": (ctypes.c_int, []),
    "d3d_meta_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_size_t]),
    "d3d_meta_destroy": (ctypes.c_int, [vp]),
    "d3d_meta_clear": (ctypes.c_int, [vp]),
    "d3d_meta_arena_used": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_size_t)]),
    "d3d_meta_set_geometry_stream": (ctypes.c_int, [vp, vp, ctypes.c_int]),
    "d3d_meta_set_plan_stream": (ctypes.c_int, [vp, vp, ctypes.c_int]),
    "d3d_geometry_async_start": (ctypes.c_int, [vp, vp, ctypes.c_int, vp, vp]),
    "d3d_geometry_async_wait": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), vp]),
    "d3d_geometry_async_finish": (ctypes.c_int, [vp]),
    "d3d_conv_ws_mode": (ctypes.c_int, [ctypes.c_int]),
    "d3d_conv_late_mode": (ctypes.c_int, [ctypes.c_int]),
    "d3d_conv_split_mode": (ctypes.c_int, [ctypes.c_int]),
    "d3d_conv_last_form": (ctypes.c_int, [c_int_p, ctypes.c_int]),
    "d3d_conv_dw_deterministic": (ctypes.c_int, [ctypes.c_int]),
    "d3d_conv_dw_thread_mode": (ctypes.c_int, [ctypes.c_int, vp, ctypes.c_size_t]),
    "d3d_conv_dw_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d3d_conv_dw_last_form": (ctypes.c_int, [c_int_p, ctypes.c_int]),
    "d3d_bn_last_form": (ctypes.c_int, [c_int_p, ctypes.c_int]),
    "d3d_roi_last_form": (ctypes.c_int, [c_int_p, ctypes.c_int]),
    "d3d_sort_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_sort_pairs": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp]),
    "d3d_conv_time_next": (ctypes.c_int, [vp, vp]),
    "d3d_input_layer_prepare": (ctypes.c_int, [vp, vp]),
    "d3d_post_scores": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp, vp, vp]),
    "d3d_post_order": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_post_gather": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]),
    "d3d_post_select_max": (ctypes.c_int, []),
    "d3d_post_select": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp,
                                       vp]),
    "d3d_roi_prepare": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_float, c_float_p, ctypes.c_int, ctypes.c_float, vp, vp,
                                       vp, vp]),
    "d3d_roi_prepare_counted": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_float, c_float_p, ctypes.c_int,
                                               ctypes.c_float, vp, vp, vp, vp]),
    "d3d_voxelize": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_int_p, vp, vp,
                                    c_int_p, vp, ctypes.c_size_t, vp]),
    "d3d_voxelize_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_augment_voxelize": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, aug_p, ctypes.c_double, c_int_p, vp, vp,
                                            c_int_p, c_double_p, vp, ctypes.c_size_t, vp]),
    "d3d_augment_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_augment_transform": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, aug_p, vp, c_double_p, vp, ctypes.c_size_t,
                                             vp]),
    "d3d_elastic_blur": (ctypes.c_int, [vp, ctypes.c_int, c_int_p, vp, vp]),
    "d3d_elastic_apply": (ctypes.c_int, [vp, ctypes.c_int, vp, c_int_p, ctypes.c_double, ctypes.c_double, c_double_p,
                                         vp, ctypes.c_size_t, vp]),
    "d3d_estimate_normals_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_estimate_normals": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, c_float_p, vp,
                                            vp, vp, ctypes.c_size_t, vp]),
    "d3d_estimate_normals_phases": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                                   c_float_p, vp, vp, vp, ctypes.c_size_t, vp, c_float_p]),
    "d3d_radius_neighbors_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_radius_neighbors": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp, vp, ctypes.c_size_t, vp,
                                            c_float_p]),
    "d3d_knn_mean_distance_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_knn_mean_distance": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_double,
                                             vp, vp, vp, vp, vp, ctypes.c_size_t, vp, c_float_p]),
    "d3d_connected_components_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_connected_components": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp, vp, vp, ctypes.c_size_t,
                                                vp, c_float_p]),
    "d3d_segment_planes_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_segment_planes": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                          vp, vp, vp, ctypes.c_size_t, vp, c_float_p]),
    "d3d_fit_planes_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_fit_planes": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp,
                                      ctypes.c_size_t, vp, c_float_p]),
    "d3d_nearest_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_nearest": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp, vp, vp,
                                   ctypes.c_size_t, vp, c_float_p]),
    "d3d_icp_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_icp": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int,
                               ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_double, vp, vp, vp, vp, vp, vp,
                               ctypes.c_size_t, vp, c_float_p]),
    "d3d_points_in_boxes": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_float,
                                           ctypes.c_float, vp, vp, vp, vp, vp]),
    "d3d_fit_boxes_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_fit_boxes": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp,
                                     vp, vp, ctypes.c_size_t, vp, c_float_p]),
    "d3d_floorplan_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d3d_floorplan_raster": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_floorplan_rooms": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp,
                                           vp, ctypes.c_size_t, vp, c_float_p]),
    "d3d_floorplan_sides": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_floorplan_points": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_manhattan_frame_scratch_bytes": (ctypes.c_size_t, []),
    "d3d_manhattan_frame": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, c_double_p, c_float_p, vp, vp, vp, vp, vp, vp,
                                           vp, ctypes.c_size_t, vp, c_float_p]),
    "d3d_global_align_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, c_int_p, ctypes.c_int]),
    "d3d_global_align": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int,
                                        vp, ctypes.c_int, vp, ctypes.c_double, c_int_p, ctypes.c_float, ctypes.c_int,
                                        ctypes.c_int, vp, vp, vp, vp, vp, ctypes.POINTER(GlobalAlignDetails), vp,
                                        ctypes.c_size_t, vp, c_float_p]),
    "d3d_voxel_downsample_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_voxel_downsample_cells": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, vp, ctypes.c_size_t,
                                                  c_int_p, vp]),
    "d3d_voxel_downsample_rows": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_int_p, vp,
                                                 ctypes.c_size_t, vp, vp, vp, vp]),
    "d3d_sample_rows_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_sample_rows": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, vp, vp, ctypes.c_size_t, vp]),
    "d3d_unproject_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d3d_unproject_count": (ctypes.c_int, [frames_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, vp, ctypes.c_size_t,
                                           c_int_p, vp]),
    "d3d_unproject_rows": (ctypes.c_int, [frames_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_int, c_int_p, vp, ctypes.c_size_t, vp, vp, vp]),
    "d3d_tsdf_table_slots": (ctypes.c_int, [ctypes.c_int]),
    "d3d_tsdf_touch": (ctypes.c_int, [frames_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, volume_p, ctypes.c_int,
                                      c_int_p, vp]),
    "d3d_tsdf_integrate": (ctypes.c_int, [frames_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, volume_p,
                                          ctypes.c_int, vp, vp]),
    "d3d_tsdf_order_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_tsdf_order": (ctypes.c_int, [vp, ctypes.c_int, vp, vp, ctypes.c_size_t, vp]),
    "d3d_tsdf_surface_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_tsdf_surface_count": (ctypes.c_int, [volume_p, ctypes.c_double, vp, ctypes.c_size_t, c_int_p, vp]),
    "d3d_tsdf_surface_rows": (ctypes.c_int, [volume_p, ctypes.c_double, ctypes.c_int, c_int_p, vp, ctypes.c_size_t, vp, vp,
                                             vp]),
    "d3d_tsdf_mesh_table": (ctypes.c_int, [vp]),
    "d3d_tsdf_mesh_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_tsdf_mesh_count": (ctypes.c_int, [volume_p, ctypes.c_double, vp, ctypes.c_size_t, c_int_p, vp]),
    "d3d_tsdf_mesh_vertices": (ctypes.c_int, [volume_p, c_int_p, vp, ctypes.c_size_t, vp, vp, vp, vp]),
    "d3d_tsdf_mesh_triangles": (ctypes.c_int, [volume_p, c_int_p, vp, ctypes.c_size_t, vp, vp]),
    "d3d_tsdf_insert_blocks": (ctypes.c_int, [vp, ctypes.c_int, volume_p, vp]),
    "d3d_render_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d3d_render_bin": (ctypes.c_int, [mesh_p, frames_p, vp, ctypes.c_size_t, c_int64_p, vp]),
    "d3d_render_fill": (ctypes.c_int, [mesh_p, frames_p, c_int64_p, vp, ctypes.c_size_t, vp, vp]),
    "d3d_render_tiles": (ctypes.c_int, [mesh_p, frames_p, ctypes.c_double, ctypes.c_double, c_int64_p, vp, ctypes.c_size_t,
                                        vp, vp, vp]),
    "d3d_input_layer_build": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, c_int_p, ctypes.c_int,
                                             ctypes.c_int, vp, c_int_p]),
    "d3d_input_layer_build_prefetch": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, c_int_p, ctypes.c_int,
                                                      ctypes.c_int, c_int_p, vp, c_int_p]),
    "d3d_input_layer_forward": (ctypes.c_int, [vp, vp, ctypes.c_int, vp, vp]),
    "d3d_input_layer_export": (ctypes.c_int, [vp, vp, vp, vp]),
    "d3d_get_n_active": (ctypes.c_int, [vp, c_int_p, c_int_p]),
    "d3d_get_spatial_locations": (ctypes.c_int, [vp, c_int_p, vp, vp]),
    "d3d_subm_prepare": (ctypes.c_int, [vp, c_int_p, c_int_p, vp, ctypes.POINTER(ctypes.c_long)]),
    "d3d_conv_prepare": (ctypes.c_int, [vp, c_int_p, c_int_p, c_int_p, c_int_p, vp, c_int_p,
                                        ctypes.POINTER(ctypes.c_long)]),
    "d3d_deconv_prepare": (ctypes.c_int, [vp, c_int_p, c_int_p, c_int_p, c_int_p, vp,
                                          ctypes.POINTER(ctypes.c_long)]),
    "d3d_export_rules": (ctypes.c_int, [vp, ctypes.c_int, c_int_p, c_int_p, c_int_p, vp, ctypes.c_long,
                                        ctypes.POINTER(ctypes.c_long), vp]),
    "d3d_bn_backward_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_input_layer_backward": (ctypes.c_int, [vp, vp, ctypes.c_int, vp, vp]),
    "d3d_sparse_to_dense_backward": (ctypes.c_int, [vp, c_int_p, vp, ctypes.c_int, vp, vp]),
    "d3d_roi_align_rotated_3d_backward": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int, vp, ctypes.c_int, ctypes.c_float,
                                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                         vp, vp]),
    "d3d_roi_align_rotated_3d_sparse_backward": (ctypes.c_int, [vp, c_int_p, vp, ctypes.c_int, c_int_p, vp,
                                                                ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                                                ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                                vp, vp]),
    "d3d_roi_align_rotated_3d_sparse_backward_deterministic": (
        ctypes.c_int, [vp, c_int_p, vp, ctypes.c_int, c_int_p, vp, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                       ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_size_t, vp]),
    "d3d_roi_align_rotated_3d_sparse_backward_deterministic_scratch_bytes": (
        ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                          ctypes.c_int]),
    "d3d_roi_align_rotated_3d_sparse_backward_bf16": (
        ctypes.c_int, [vp, c_int_p, vp, ctypes.c_int, c_int_p, vp, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                       ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_size_t, vp]),
    "d3d_roi_align_rotated_3d_sparse_backward_bf16_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16": (
        ctypes.c_int, [vp, c_int_p, vp, ctypes.c_int, c_int_p, vp, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                       ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_size_t, vp]),
    "d3d_roi_align_rotated_3d_sparse_backward_deterministic_bf16_scratch_bytes": (
        ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                          ctypes.c_int]),
    "d3d_bn_batch_stats": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp]),
    "d3d_bn_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_add": (ctypes.c_int, [vp, vp, vp, ctypes.c_size_t, vp]),
    "d3d_sparse_to_dense_forward": (ctypes.c_int, [vp, c_int_p, vp, ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_roi_align_rotated_3d_forward": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_int, ctypes.c_int, vp, ctypes.c_int,
                                                        ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_roi_align_rotated_3d_sparse_forward": (ctypes.c_int, [vp, c_int_p, vp, ctypes.c_int, c_int_p, vp,
                                                               ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                                               ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                               vp, ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_roi_align_rotated_3d_sparse_forward_levels": (ctypes.c_int, [vp, ctypes.c_int, c_int_p, ctypes.POINTER(vp),
                                                                      ctypes.c_int, c_float_p, vp, ctypes.c_int,
                                                                      ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                                      ctypes.c_int, vp, ctypes.c_int, vp, vp]),
    "d3d_roi_align_rotated_3d_sparse_forward_bf16": (ctypes.c_int, [vp, c_int_p, vp, ctypes.c_int, c_int_p, vp,
                                                                    ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                                                    ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                                    vp, ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_roi_align_rotated_3d_sparse_forward_levels_bf16": (ctypes.c_int, [vp, ctypes.c_int, c_int_p, ctypes.POINTER(vp),
                                                                           ctypes.c_int, c_float_p, vp, ctypes.c_int,
                                                                           ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                                           ctypes.c_int, vp, ctypes.c_int, vp, vp]),
    "d3d_rotate_iou_eval": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_boxes_iou_3d": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                        ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_match_segments": (ctypes.c_int, [vp, c_int_p, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_float),
                                          ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_float), vp, vp, vp, ctypes.c_size_t, vp]),
    "d3d_match_segments_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_rotate_nms_3d_batched": (ctypes.c_int, [vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                 ctypes.c_float, ctypes.c_float, ctypes.c_int, vp, vp, vp,
                                                 ctypes.c_size_t, vp]),
    "d3d_nms_batched_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_nms_sweep_mode": (ctypes.c_int, [ctypes.c_int]),
    "d3d_nms_last_form": (ctypes.c_int, [c_int_p, ctypes.c_int]),
    "d3d_rotate_nms_3d": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_float, vp, vp, c_int_p, vp, ctypes.c_size_t, vp]),
    "d3d_rotate_nms_3d_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_topk_segments": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, c_float_p, c_int_p, vp, ctypes.c_int, vp,
                                         ctypes.c_float, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]),
    "d3d_topk_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "d3d_topk_max": (ctypes.c_int, []),
    "d3d_anchors": (ctypes.c_int, [vp, c_int_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_float), ctypes.c_float, vp, vp]),
    "d3d_anchors_maps": (ctypes.c_int, [vp, ctypes.c_int, c_int_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_float), ctypes.c_float, vp, vp]),
    "d3d_rpn_head": (ctypes.c_int, [ctypes.POINTER(vp), c_int_p, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp,
                                    ctypes.c_int, vp, vp, vp]),
    "d3d_rpn_head_bf16": (ctypes.c_int, [ctypes.POINTER(vp), c_int_p, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp,
                                         ctypes.c_int, vp, vp, vp]),
    "d3d_mlp_heads": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int, vp, vp, vp]),
    "d3d_rotate_nms_3d_sorted": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_float, ctypes.c_int, vp, vp, vp,
                                                ctypes.c_size_t, vp]),
    "d3d_nms_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "d3d_box_decode": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_float,
                                      vp, vp]),
    "d3d_box_decode_classes": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                              ctypes.c_float, vp, vp]),
    "d3d_box_decode_rows": (ctypes.c_int, [vp, vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_float,
                                           vp, vp]),
    "d3d_gather_kept": (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_int, ctypes.c_float, vp, vp, vp, vp]),
    "d3d_plan_export": (ctypes.c_int, [vp, ctypes.c_int, c_int_p, c_int_p, c_int_p, vp, vp, vp, c_int_p, vp]),
    "d3d_plan_last_form": (ctypes.c_int, [c_int_p, ctypes.c_int]),
    "d3d_subm_probe_mode": (ctypes.c_int, [ctypes.c_int]),
    "d3d_plan_stats": (ctypes.c_int, [vp, ctypes.c_int, c_int_p, c_int_p, c_int_p, ctypes.POINTER(ctypes.c_long),
                                      ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long), vp]),
    # storage-type aware forms (d3d_dtype: 0 fp32, 1 bf16)
    "d3d_packed_weight_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d3d_pack_conv_weight_dt": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp]),
    "d3d_subm_conv_forward_dt": (ctypes.c_int, [vp, c_int_p, c_int_p, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp,
                                                ctypes.c_int, vp, ctypes.POINTER(ctypes.c_double), bn_p]),
    "d3d_conv_forward_dt": (ctypes.c_int, [vp, c_int_p, c_int_p, c_int_p, c_int_p, vp, ctypes.c_int, vp, ctypes.c_int,
                                           vp, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_double), bn_p]),
    "d3d_deconv_forward_dt": (ctypes.c_int, [vp, c_int_p, c_int_p, c_int_p, c_int_p, vp, ctypes.c_int, vp, ctypes.c_int,
                                             vp, vp, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_double), bn_p]),
    "d3d_conv_group_forward": (ctypes.c_int, [vp, ctypes.POINTER(ConvDesc), ctypes.c_int, vp]),
    "d3d_conv_bf16_tuning": (ctypes.c_int, [ctypes.c_int, ctypes.c_long]),
    "d3d_bn_stats_from_partials": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                                  vp, vp, vp, ctypes.c_size_t, vp]),
    "d3d_bn_batch_invstd_dt": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp, vp, vp,
                                              ctypes.c_size_t, ctypes.c_int, vp]),
    "d3d_rows_to_bf16": (ctypes.c_int, [vp, ctypes.c_long, ctypes.c_int, ctypes.c_int, vp, vp]),
    "d3d_bn_apply_dt": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_float,
                                       ctypes.c_int, vp]),
    "d3d_pack_conv_weight_transposed_dt": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                          vp, ctypes.c_int, vp]),
    "d3d_subm_conv_backward_dt": (ctypes.c_int, [vp, c_int_p, c_int_p, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int,
                                                 vp, vp, vp, ctypes.c_int, vp]),
    "d3d_conv_backward_dt": (ctypes.c_int, [vp, c_int_p, c_int_p, c_int_p, c_int_p, vp, ctypes.c_int, ctypes.c_int, vp,
                                            ctypes.c_int, vp, vp, vp, ctypes.c_int, vp]),
    "d3d_deconv_backward_dt": (ctypes.c_int, [vp, c_int_p, c_int_p, c_int_p, c_int_p, vp, ctypes.c_int, ctypes.c_int, vp,
                                              ctypes.c_int, vp, vp, vp, ctypes.c_int, vp]),
    "d3d_bn_forward_dt": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.c_float,
                                         ctypes.c_float, ctypes.c_int, ctypes.c_float, vp, ctypes.c_size_t, ctypes.c_int,
                                         vp]),
    "d3d_bn_backward_dt": (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp,
                                          ctypes.c_float, vp, ctypes.c_size_t, ctypes.c_int, vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGS.keys())


class D3DError(RuntimeError):
    pass


def lib():
    """Loads the HIP library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise D3DError(
                f"{LIB_PATH} not found: build it with `python -m detection_3d_amd.build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().d3d_last_error()
        raise D3DError(f"libd3d_hip error {rc}: {msg.decode() if msg else ''}")


_INTS = {}     # tuple -> ctypes int array; the library only reads these arrays


def ints(values):
    if type(values) is tuple:
        a = _INTS.get(values)
        if a is None:
            if len(_INTS) > 4096:
                _INTS.clear()
            a = _INTS[values] = (ctypes.c_int * len(values))(*values)
        return a
    values = [int(v) for v in values]
    return (ctypes.c_int * len(values))(*values)


def floats(values):
    values = [float(v) for v in values]
    return (ctypes.c_float * len(values))(*values)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def raw_stream(device=None):
    """hipStream_t of torch's current stream as an int (torch.cuda.current_stream costs ~10 us of Python per
    call, and every library call needs the stream)."""
    if _RAW_STREAM is None or _GET_DEVICE is None:
        return torch.cuda.current_stream(device).cuda_stream
    idx = None if device is None else (device if isinstance(device, int) else device.index)
    return _RAW_STREAM(_GET_DEVICE() if idx is None else idx)


def stream_of(device=None):
    return ctypes.c_void_p(raw_stream(device))


def deterministic():
    """torch.use_deterministic_algorithms(True) is in force: the library's ops take their fixed-order forms.  Read at
    call time, so switching the flag takes effect on the next call."""
    return torch.are_deterministic_algorithms_enabled()


def fills_uninitialized():
    """torch fills every new tensor (torch.empty, resize_) with NaN / the largest integer on the current stream: in
    deterministic mode with torch.utils.deterministic.fill_uninitialized_memory (its default)."""
    return torch.are_deterministic_algorithms_enabled() and torch.utils.deterministic.fill_uninitialized_memory


def alert_not_deterministic(op):
    """What torch's own ops do in deterministic mode when they have no deterministic form: raise (or, with
    warn_only=True, warn and go on with the nondeterministic form)."""
    msg = (f"{op} does not have a deterministic implementation, but you set "
           "'torch.use_deterministic_algorithms(True)'.")
    if torch.is_deterministic_algorithms_warn_only_enabled():
        import warnings
        warnings.warn(msg)
        return
    raise RuntimeError(msg)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise D3DError("this op runs on the MI355X only: tensor is on %s (no CPU fallback)" % t.device)
        if t is not None and not t.is_contiguous():
            raise D3DError("tensor must be contiguous")


_HOST_WORDS = {}
_HOST_WORD_RING = 8
_HOST_WORD_BLOCKING = os.environ.get("D3D_COUNT_EVENT_BLOCKING", "1") != "0"


def host_word(device, tag):
    """-> (pinned int32 [1] host tensor, event): the next slot of a small ring kept per (device, current stream, tag), so
    that a deferred read-back (PaddedProposals.resolve) still finds its own word and event when further counts have been
    requested on the same stream meanwhile (up to _HOST_WORD_RING outstanding ones).  A kernel stores a count to the word
    (pinned host memory is device-visible at the same address), the caller records the event behind that launch and
    the host waits for the event alone: no copy engine between the kernel and the host, and launches enqueued behind the
    event do not hold the host up."""
    key = (device.index, raw_stream(device), tag)
    ring = _HOST_WORDS.get(key)
    if ring is None:
        ring = _HOST_WORDS[key] = [[], 0]
    slots, nxt = ring
    if len(slots) < _HOST_WORD_RING:
        slots.append((torch.zeros(1, dtype=torch.int32).pin_memory(), torch.cuda.Event(blocking=_HOST_WORD_BLOCKING)))
        return slots[-1]
    ring[1] = (nxt + 1) % _HOST_WORD_RING
    return slots[nxt]
