"""ctypes loader for libspherehand_hip.so (the C ABI in include/spherehand_hip.h).

There is NO fallback: if the HIP library is missing or fails to load, importing
any op raises.  Build it with ``python -m spherehand_amd.build``.
"""
import ctypes
import os

# torch FIRST: the wheel bundles its own ROCm runtime (torch/lib/libamdhip64.so,
# SONAME libamdhip64.so.7).  Loaded after torch, our library's NEEDED
# libamdhip64.so.7 binds to that same runtime; loaded before torch, the process
# would end up with two HIP runtimes (/opt/rocm's and torch's) and kernels
# launched on torch's streams fail with hipErrorNoDevice.
import torch  # noqa: F401  (device memory, streams: the plumbing this library sits on)

_PKG = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_PKG, "libspherehand_hip.so")
ABI_VERSION = 23

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float

# name -> argtypes; every symbol include/spherehand_hip.h declares
SIGNATURES = {
    "shr_abi_version": ([], _i),
    "shr_error_string": ([_i], ctypes.c_char_p),
    "shr_device_info": ([ctypes.c_char_p, _i, ctypes.POINTER(_i)], _i),
    "shr_sphere_raster_fwd": ([_vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_sphere_raster_fwd_ex": ([_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp], _i),
    "shr_keypoint_spheres_fwd": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp], _i),
    "shr_keypoint_spheres_bwd": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp], _i),
    "shr_sphere_raster_bwd": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp], _i),
    "shr_set_tuning": ([_i, _i], _i),
    "shr_data_to_model": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_data_to_model_indexed": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_data_to_model_parts": ([_i, _i, _i], _i),
    "shr_data_to_model_partial": ([_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_data_to_model_points_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_data_to_model_compact": ([_vp, _i, _i, _i, _vp, _vp], _i),
    "shr_mv_project_compact": ([_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp], _i),
    "shr_data_to_model_from_points": ([_vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_data_to_model_from_points_indexed": ([_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_data_to_model_from_points_ordered": ([_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_mv_loss_combine": ([_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "shr_sphere_raster_mse_regions": ([_i, _i], _i),
    "shr_pair_losses": ([_vp, ctypes.c_longlong, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_mv_consistency": ([_vp, _vp, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_depth_resample": ([_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp], _i),
    "shr_soft_argmax_supported": ([_i, _i, _i], _i),
    "shr_soft_argmax_fwd": ([_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, _i, _i, _i, _i, _f, _f, _f, _f, _f,
                             _vp, _vp], _i),
    "shr_soft_argmax_bwd": ([_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, _i, _i, _i, _i, _f, _f, _f, _f, _f,
                             _vp, _vp, _vp], _i),
    "shr_heatmap_paint": ([_vp, _i, _i, _f, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp], _i),
    "shr_depth_noise": ([_vp, _vp, _i, _i, _i, _f, _f, _vp, _vp], _i),
    "shr_synth_pose_fwd": ([_vp, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp], _i),
    "shr_mesh_render_post_fwd": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp, _i, _i, _i, _f, _f, _vp, _f, _f,
                                 _vp, _vp, _vp, _vp, _vp], _i),
    "shr_mesh_render_one_launch": ([_i, _i, _i, _i, _i], _i),
    "shr_hand_synth_one_launch": ([_i, _i, _i, _i, _i, _i, _i], _i),
    "shr_hand_synth_fwd": ([_vp, _i, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _i, _i, _i, _f, _f, _i, _f, _f,
                           _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_heatmap_render_fwd": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _i, _f, _f, _f, _f, _f, _f, _f, _vp, _vp,
                               _vp, _vp], _i),
    "shr_group_norm_relu_supported": ([_i, _i], _i),
    "shr_group_norm_relu_fwd": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp], _i),
    "shr_group_norm_relu_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_group_norm_relu_bf16_fwd": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp], _i),
    "shr_group_norm_relu_bf16_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_sphere_raster_mse": ([_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_sphere_raster_mse_indexed": ([_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_sphere_raster_mse_ordered": ([_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_mutual_project_fwd": ([_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp], _i),
    "shr_mutual_project_bwd": ([_vp, _vp, _vp, _i, _i, _i, _vp, _vp], _i),
    "shr_tri_raster_fwd": ([_vp, _i, _i, _i, _i, _vp, _vp], _i),
    "shr_tri_raster_indexed_fwd": ([_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "shr_mesh_depth_fwd": ([_vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp], _i),
    "shr_mesh_render_fwd": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "shr_lbs_project": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp], _i),
    "shr_mesh_depth_owner_fwd": ([_vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "shr_mesh_depth_bwd_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_mesh_depth_bwd": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_lbs_project_bwd": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp, _vp], _i),
    "shr_tri_raster_owner_fwd": ([_vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_tri_raster_indexed_owner_fwd": ([_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_tri_raster_bwd_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_tri_raster_indexed_bwd_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_tri_raster_bwd": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_tri_raster_indexed_bwd": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_tri_antialias_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "shr_tri_antialias_bwd_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_tri_antialias_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_tri_antialias_maps_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "shr_tri_antialias_maps_bwd_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_tri_antialias_maps_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_tri_interp_fwd": ([_vp, _vp, _vp, _vp, ctypes.c_longlong, _i, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "shr_tri_interp_bwd_workspace_bytes": ([_i, _i, _i, _i, _i], ctypes.c_longlong),
    "shr_tri_interp_bwd": ([_vp, _vp, _vp, _vp, ctypes.c_longlong, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_tri_vertex_normals_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "shr_tri_vertex_normals_bwd_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_tri_vertex_normals_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp,
                                    _vp], _i),
    "shr_unit3_maps_fwd": ([_vp, _i, _i, _i, _vp, _vp], _i),
    "shr_unit3_maps_bwd": ([_vp, _vp, _i, _i, _i, _vp, _vp], _i),
    "shr_dt_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_dt_fwd": ([_vp, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "shr_dt_sample_fwd": ([_vp, _i, _i, _i, _vp, _i, _i, _f, _vp, _vp, _vp], _i),
    "shr_dt_sample_bwd": ([_vp, _vp, _i, _i, _i, _vp, _vp], _i),
    "shr_dt_nearest_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_dt_nearest_fwd": ([_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp], _i),
    "shr_sil_cover_fwd": ([_vp, _f, _vp, _i, _i, _i, _f, _vp, _vp], _i),
    "shr_sil_cover_bwd_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_sil_cover_bwd": ([_vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp], _i),
    "shr_mesh_d2m_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_mesh_d2m_fwd": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp], _i),
    "shr_mesh_d2m_bwd_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_mesh_d2m_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp], _i),
    "shr_depth_normals_fwd": ([_vp, _i, _i, _i, _f, _f, _f, _f, _vp, _vp], _i),
    "shr_depth_normals_bwd": ([_vp, _vp, _i, _i, _i, _f, _f, _f, _f, _vp, _vp], _i),
    "shr_fk_fwd":([_vp, _i, _vp, _vp, _vp, _vp], _i),
    "shr_fk_bwd": ([_vp, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_pose_spheres_fwd": ([_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp], _i),
    "shr_pose_spheres_bwd": ([_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp], _i),
    "shr_lbs_vertices_bwd": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp], _i),
    "shr_pose_vertices_fwd": ([_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp], _i),
    "shr_pose_vertices_bwd": ([_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp], _i),
    "shr_pose_keypoints_jacobian": ([_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp], _i),
    "shr_pose_ik_fwd": ([_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _f, _vp, _vp, _vp, _vp], _i),
    "shr_pose_ik_bwd": ([_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp], _i),
    "shr_pose_icp_normal_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_pose_icp_normal": ([_vp] * 11 + [_i] * 6 + [_f] * 6 + [_vp] * 6, _i),
    "shr_pose_lm_state_bytes": ([_i], ctypes.c_longlong),
    "shr_pose_lm_begin": ([_vp, _i, _f, _vp, _vp, _vp], _i),
    "shr_pose_lm_step": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "shr_view_vertices_fwd": ([_vp, _vp, _i, _i, _i, _vp, _vp], _i),
    "shr_pose_icp_normal_views_workspace_bytes": ([_i, _i, _i, _i], ctypes.c_longlong),
    "shr_pose_icp_normal_views": ([_vp] * 12 + [_i] * 7 + [_f] * 6 + [_vp] * 6, _i),
    "shr_sphere_icp_normal_workspace_bytes": ([_i, _i, _i, _i, _i], ctypes.c_longlong),
    "shr_sphere_icp_normal": ([_vp] * 5 + [_i] * 5 + [_f] * 6 + [_vp] * 9, _i),
    "shr_sphere_render_normal_workspace_bytes": ([_i, _i, _i, _i, _i], ctypes.c_longlong),
    "shr_sphere_render_normal": ([_vp] * 5 + [_i] * 5 + [_f] * 8 + [_i] + [_vp] * 9, _i),
    "shr_sphere_prior_normal_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_sphere_prior_normal": ([_vp] * 6 + [_f, _f, _vp, _vp, _f] + [_i] * 4 + [_vp] * 7, _i),
    "shr_sphere_collision_normal_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_sphere_collision_normal": ([_vp] * 5 + [_f] + [_i] * 4 + [_vp] * 7, _i),
    "shr_pose_vae_blob_floats": ([], _i),
    "shr_pose_vae_normal_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_pose_vae_normal": ([_vp] * 3 + [_i, _f, _f] + [_i] * 3 + [_vp] * 8, _i),
    "shr_sphere_temporal_normal_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_sphere_temporal_normal": ([_vp] * 3 + [_f, _f] + [_i] * 4 + [_vp] * 7, _i),
    "shr_pose_lm_seq_state_bytes": ([_i], ctypes.c_longlong),
    "shr_pose_lm_seq_workspace_bytes": ([_i], ctypes.c_longlong),
    "shr_pose_lm_seq_begin": ([_vp, _i, _i, _f, _vp, _vp, _vp], _i),
    "shr_pose_lm_seq_step": ([_vp] * 8 + [_i] * 3 + [_vp] * 6, _i),
    "shr_sphere_accel_normal_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_sphere_accel_normal": ([_vp] * 3 + [_f, _f] + [_i] * 5 + [_vp] * 8, _i),
    "shr_pose_lm_seq2_state_bytes": ([_i], ctypes.c_longlong),
    "shr_pose_lm_seq2_workspace_bytes": ([_i], ctypes.c_longlong),
    "shr_pose_lm_seq2_begin": ([_vp, _i, _i, _f, _vp, _vp, _vp], _i),
    "shr_pose_lm_seq2_step": ([_vp] * 9 + [_i] * 3 + [_vp] * 6, _i),
    "shr_pose_lm_seq2_covariance_workspace_bytes": ([_i], ctypes.c_longlong),
    "shr_pose_lm_seq2_covariance": ([_vp] * 5 + [_i] * 3 + [_vp] * 5, _i),
    "shr_pose_window_marginalize_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_pose_window_marginalize": ([_vp] * 8 + [_i] * 2 + [_vp] * 7, _i),
    "shr_pose_window_prior_normal_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "shr_pose_window_prior_normal": ([_vp] * 6 + [_i] * 4 + [_vp] * 6, _i),
    "shr_sphere_icp_radii_normal_workspace_bytes": ([_i, _i, _i, _i, _i], ctypes.c_longlong),
    "shr_sphere_icp_radii_normal": ([_vp] * 5 + [_i] * 6 + [_f] * 6 + [_vp] * 12, _i),
    "shr_pose_lm_shared_state_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_pose_lm_shared_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "shr_pose_lm_shared_begin": ([_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp], _i),
    "shr_pose_lm_shared_step": ([_vp] * 13 + [_i] * 4 + [_vp] * 8, _i),
    "shr_selftest_sqrt":([ctypes.c_uint, ctypes.c_uint, _vp, _vp], _i),
    "shr_selftest_division": ([ctypes.c_uint, ctypes.c_uint, _vp, _vp], _i),
    "shr_selftest_launch_floor": ([_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp], _i),
}

_lib = None


class SphereHandLibraryError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise SphereHandLibraryError(
            "%s not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m spherehand_amd.build`." % SO_PATH)
    try:
        h = ctypes.CDLL(SO_PATH)
    except OSError as e:  # pragma: no cover
        raise SphereHandLibraryError("cannot load %s: %s" % (SO_PATH, e))
    for name, (args, res) in SIGNATURES.items():
        try:
            fn = getattr(h, name)
        except AttributeError:
            raise SphereHandLibraryError("%s does not export %s (stale build?)" % (SO_PATH, name))
        fn.argtypes = args
        fn.restype = res
    v = h.shr_abi_version()
    if v != ABI_VERSION:
        raise SphereHandLibraryError("ABI version %d, expected %d: rebuild" % (v, ABI_VERSION))
    _lib = h
    return h


def check(rc, what):
    if rc != 0:
        msg = lib().shr_error_string(rc).decode()
        raise RuntimeError("%s failed: %s (code %d)" % (what, msg, rc))
