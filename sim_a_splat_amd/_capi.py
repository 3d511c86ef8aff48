"""ctypes binding of libsas_hip.so (include/sim_a_splat_amd.h).

There is no CPU fallback: if the shared library is missing or fails to load, importing this
module's ``lib()`` raises.  The oracle under ``oracle/`` is never imported from here.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

_PKG = Path(__file__).resolve().parent
# SAS_LIB_PATH points the binding at another build of the same library (the -DSAS_TUNE_* / -DSAS_DEBUG_BOUNDS
# variants under variants/, for A/B measurements and the bounds-checked test run)
LIB_PATH = Path(os.environ.get("SAS_LIB_PATH") or (_PKG / "libsas_hip.so"))

SAS_DEPTH_FILL_MAX = 1
SAS_ASYNC = 2
SAS_FAST_EXP = 4
SAS_TIMING = 8
SAS_FULL_SORT = 16
SAS_TIME_TILES = 32
SAS_MESH_SURFACE = 64
SAS_LIFT_ONE = 2 ** 32   # the fixed-point unit of a vote (sas_lift_labels)
SAS_LIFT_FEATURE_ONE = 2 ** 24   # the fixed-point unit of a feature-lift weight (sas_lift_features)
SAS_QUERY_CHUNK = 256   # triangles the mesh-query kernel stages in LDS at a time (csrc/sas_internal.h)
SAS_CLOUD_RESIDENT = 16384   # survivors per cloud the sampling kernel keeps in registers (csrc/sas_internal.h)
SAS_FUSE_THREADS = 256   # voxels per workgroup of the fusion kernel (csrc/sas_internal.h)
SAS_MATCH_CHUNK = 256   # targets the point-matching kernel stages in LDS at a time (csrc/sas_internal.h)
SAS_ORDER_TILE = 2048   # keys a workgroup of the storage-order sort ranks (csrc/sas_internal.h)
SAS_ORDER_SCAN_ROUND = 1024   # entries of its [256][tiles] histogram table the one-workgroup scan takes per round (csrc/sas_internal.h)
SAS_KNN_MAX_K = 8   # neighbours per point sas_knn_points finds at most (csrc/sas_internal.h)
SAS_KNN_CROSS_MAX_NODES = 65536   # nodes sas_knn_cross and sas_scene_deform take at most (csrc/sas_internal.h)
SAS_SKIN_MAX_K = 8   # entries per Gaussian of a skin at most (csrc/sas_internal.h)
SAS_SKIN_LDS_BYTES = 16384   # node records the deformation kernel stages in LDS at most: the SAS_SKIN_LDS budget's default (csrc/sas_internal.h)
SAS_SKIN_GRAD_LDS_BYTES = 131072   # per-node sums the deformation's adjoint keeps in LDS at most: the SAS_SKIN_GRAD_LDS budget's default (csrc/sas_internal.h)
SAS_KNN_RING_LIMIT = 4  # rings of cells its grid search visits before a point goes to the brute-force kernel (csrc/sas_internal.h)
SAS_NODES_MAX_K = 8   # neighbours per node sas_nodes_rigidity takes at most (csrc/sas_internal.h)
SAS_NODES_FIT_MAX_LANES = 1 << 30   # (step, node) pairs sas_nodes_fit_rigid takes at most (csrc/sas_internal.h)
SAS_MAX_POSE_GRAD_GROUPS = 32   # groups whose pose gradient one sas_render_backward_poses call forms

STAGE_NAMES = ("project", "scan", "scatter", "sort", "blend", "tail", "total")
STAT_NAMES = ("n_visible", "n_isect", "max_tile_len", "capacity", "regrows", "window_misses", "fallback_tiles", "quad_layout", "launch_views", "n_keys")

# every symbol include/sim_a_splat_amd.h declares
EXPORTS = (
    "sas_create", "sas_destroy", "sas_scene_upload", "sas_set_group_poses", "sas_set_link_constants", "sas_set_link_poses", "sas_get_group_poses", "sas_link_attached_frame", "sas_link_group_poses", "sas_attached_frame", "sas_camera_matrices", "sas_render_cameras_host", "sas_render", "sas_render_rgbd", "sas_scene_features", "sas_render_features", "sas_scene_meshes", "sas_scene_mesh_features", "sas_scene_mesh_vertex_attributes", "sas_query_meshes", "sas_match_points", "sas_sample_points", "sas_fuse_depth", "sas_render_batch", "sas_render_batch_host", "sas_render_batch_posed", "sas_render_batch_host_posed", "sas_render_batch_labels", "sas_render_batch_labels_posed", "sas_lift_labels", "sas_lift_features", "sas_render_backward_screen", "sas_render_backward", "sas_render_backward_poses", "sas_scene_adam_step", "sas_scene_adam_reset", "sas_density_accumulate", "sas_scene_densify", "sas_scene_densify_times", "sas_scene_reset_opacity", "sas_scene_mcmc_noise", "sas_scene_mcmc_refine", "sas_photometric_loss", "sas_scene_read", "sas_storage_order", "sas_scene_order", "sas_knn_points", "sas_knn_last_counts", "sas_knn_cross", "sas_scene_skin", "sas_scene_skin_read", "sas_scene_deform", "sas_scene_deform_backward", "sas_scene_deform_backward_rest", "sas_scene_adam_step_rest", "sas_nodes_rigidity", "sas_nodes_twist_step", "sas_nodes_fit_rigid", "sas_wait", "sas_frames_completed",
    "sas_last_error", "sas_stage_times", "sas_stage_time_means", "sas_frame_stats", "sas_read_projection", "sas_read_tile_lists",
    "sas_version",
)

_lib: Optional[ctypes.CDLL] = None

SAS_ADAM_VISIBLE_ONLY = 1
SAS_DEFORM_REST_BOUND_ONLY = 1


class AdamConfig(ctypes.Structure):
    """sas_adam_config of include/sim_a_splat_amd.h."""
    _fields_ = [(k, ctypes.c_float) for k in ("lr_means", "lr_opacities", "lr_sh_dc", "lr_sh_rest", "lr_quats", "lr_scales", "beta1", "beta2", "eps")] + \
               [("step", ctypes.c_int), ("flags", ctypes.c_uint)]


SAS_DENSIFY_GROW = 1
SAS_DENSIFY_PRUNE_OPACITY = 2
SAS_DENSIFY_PRUNE_SCALE = 4


class DensifyConfig(ctypes.Structure):
    """sas_densify_config of include/sim_a_splat_amd.h."""
    _fields_ = [(k, ctypes.c_float) for k in ("grow_grad2d", "grow_scale3d", "prune_opacity", "prune_scale3d", "scene_extent", "split_factor")] + \
               [("max_gaussians", ctypes.c_int64), ("seed", ctypes.c_uint), ("flags", ctypes.c_uint)]


class McmcConfig(ctypes.Structure):
    """sas_mcmc_config of include/sim_a_splat_amd.h."""
    _fields_ = [("cap_max", ctypes.c_int64), ("grow_factor", ctypes.c_double), ("min_opacity", ctypes.c_float), ("seed", ctypes.c_uint)]


class NodeStepConfig(ctypes.Structure):
    """sas_node_step_config of include/sim_a_splat_amd.h."""
    _fields_ = [(k, ctypes.c_double) for k in ("lr_rot", "lr_trans", "beta1", "beta2", "c1", "c2", "eps", "gain1", "gain2")]


class SasError(RuntimeError):
    """Raised for any non-zero status of the C ABI (the reference raises RuntimeError too,
    sim_a_splat/env/splat/splat_env_wrapper.py:93-94)."""


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise SasError(
            f"{LIB_PATH} is missing: build it with `python -m sim_a_splat_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for the render path.")
    # ONE HIP runtime per process: the library is handed torch's device pointers and streams, so it has to resolve libamdhip64 to the
    # copy torch has loaded.  Loaded BEFORE torch it binds the system copy instead, and sas_create then finds no device
    # (SAS_ERR_NO_DEVICE) once torch has brought its own -- so torch comes first whenever it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:   # a C / ctypes consumer without torch: the system runtime is the only one
        pass
    L = ctypes.CDLL(str(LIB_PATH))
    vp, ci, cu, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_int64
    L.sas_create.argtypes = [ci, ctypes.POINTER(vp)]
    L.sas_destroy.argtypes = [vp]
    L.sas_scene_upload.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, ci, vp, ci]
    L.sas_set_group_poses.argtypes = [vp, ci, vp]
    L.sas_set_link_constants.argtypes = [vp, ci, ctypes.c_double, vp, vp, vp, vp, vp, vp]
    L.sas_set_link_poses.argtypes = [vp, ci, vp, vp, vp]
    L.sas_get_group_poses.argtypes = [vp, ci, vp]
    cd = ctypes.c_double
    L.sas_link_attached_frame.argtypes = [vp, vp, vp, vp, vp, vp]
    L.sas_link_group_poses.argtypes = [ci, cd, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sas_attached_frame.argtypes = [cd, vp, vp, vp, vp, vp, vp, vp]
    L.sas_camera_matrices.argtypes = [ci, vp, vp, cd, ci, ci, vp, vp]
    L.sas_render_cameras_host.argtypes = [vp, ci, vp, vp, cd, ci, ci, vp, cu, vp, vp]
    L.sas_render.argtypes = [vp, vp, vp, ci, ci, vp, cu, vp, vp, vp, vp, vp]
    L.sas_render_rgbd.argtypes = [vp, vp, vp, ci, ci, vp, cu, vp, vp, vp, vp, vp, vp, vp]
    L.sas_scene_features.argtypes = [vp, i64, ci, vp]
    L.sas_scene_meshes.argtypes = [vp, i64, vp, i64, vp, vp, vp, ctypes.c_float, ctypes.c_float]
    L.sas_scene_mesh_features.argtypes = [vp, i64, ci, vp]
    L.sas_scene_mesh_vertex_attributes.argtypes = [vp, i64, vp, vp]
    L.sas_query_meshes.argtypes = [vp, i64, vp, i64, vp, i64, vp, ci, vp, ctypes.c_float, vp, vp, vp]
    L.sas_match_points.argtypes = [vp, i64, vp, i64, vp, vp, ctypes.c_float, ci, vp, vp, vp, vp]
    L.sas_sample_points.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, ctypes.c_float, ci, ci, cu, vp, vp, vp, vp, vp, vp]
    cf = ctypes.c_float
    L.sas_fuse_depth.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, cf, vp, cf, cf, cf, cf, cu, vp, vp, vp, vp]
    L.sas_render_features.argtypes = [vp, vp, vp, ci, ci, vp, vp, cu, vp, vp, vp, vp, vp]
    L.sas_render_batch.argtypes = [vp, ci, vp, vp, ci, ci, vp, cu, vp, vp, vp, vp, vp]
    L.sas_render_batch_host.argtypes = [vp, ci, vp, vp, ci, ci, vp, cu, vp, vp]
    L.sas_render_batch_posed.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ci, vp, cu, vp, vp, vp, vp, vp]
    L.sas_render_batch_host_posed.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ci, vp, cu, vp, vp]
    L.sas_render_batch_labels.argtypes = [vp, ci, vp, vp, ci, ci, vp, cf, cu, vp, vp, vp, vp, vp, vp]
    L.sas_render_batch_labels_posed.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ci, vp, cf, cu, vp, vp, vp, vp, vp, vp]
    L.sas_lift_labels.argtypes = [vp, ci, vp, vp, ci, ci, vp, ci, cu, vp, vp, vp]
    L.sas_lift_features.argtypes = [vp, ci, vp, vp, ci, ci, vp, ci, cf, vp, cu, vp, vp, vp]
    L.sas_render_backward_screen.argtypes = [vp, vp, vp, ci, ci, cu, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sas_render_backward.argtypes = [vp, vp, vp, ci, ci, cu, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sas_render_backward_poses.argtypes = [vp, vp, vp, ci, ci, cu, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp]
    L.sas_scene_adam_step.argtypes = [vp, ctypes.POINTER(AdamConfig), vp, vp, vp, vp, vp, vp]
    L.sas_scene_adam_reset.argtypes = [vp]
    L.sas_density_accumulate.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
    L.sas_scene_densify.argtypes = [vp, ctypes.POINTER(DensifyConfig), vp, vp, vp, vp, vp]
    L.sas_scene_densify_times.argtypes = [vp, vp, ci]
    L.sas_scene_reset_opacity.argtypes = [vp, cf, vp]
    L.sas_scene_mcmc_noise.argtypes = [vp, cf, ci, cu, vp]
    L.sas_scene_mcmc_refine.argtypes = [vp, ctypes.POINTER(McmcConfig), vp, vp, vp]
    L.sas_photometric_loss.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, cf, vp, vp, vp, vp]
    L.sas_scene_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.sas_storage_order.argtypes = [vp, i64, vp, vp, vp, vp]
    L.sas_scene_order.argtypes = [vp, vp]
    L.sas_knn_points.argtypes = [vp, i64, vp, ci, vp, vp, vp]
    L.sas_knn_last_counts.argtypes = [vp, vp, ci]
    L.sas_knn_cross.argtypes = [vp, i64, vp, i64, vp, ci, cf, vp, vp, vp]
    L.sas_scene_skin.argtypes = [vp, ci, vp, vp, vp]
    L.sas_scene_skin_read.argtypes = [vp, vp, vp]
    L.sas_scene_deform.argtypes = [vp, ci, vp, vp]
    L.sas_scene_deform_backward.argtypes = [vp, vp, vp, vp, vp, vp]
    L.sas_scene_deform_backward_rest.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint, vp]
    L.sas_scene_adam_step_rest.argtypes = L.sas_scene_adam_step.argtypes
    L.sas_nodes_rigidity.argtypes = [vp, i64, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.sas_nodes_twist_step.argtypes = [vp, i64, vp, vp, vp, cd, vp, vp, vp, vp, ctypes.POINTER(NodeStepConfig), vp]
    L.sas_nodes_fit_rigid.argtypes = [vp, ci, i64, vp, vp, ci, vp, vp, vp, vp]
    L.sas_wait.argtypes = [vp]
    L.sas_frames_completed.argtypes = [vp, vp, vp]
    L.sas_last_error.argtypes = [vp]
    L.sas_last_error.restype = ctypes.c_char_p
    L.sas_stage_times.argtypes = [vp, vp, ci]
    L.sas_stage_time_means.argtypes = [vp, vp, ci, vp, ci]
    L.sas_frame_stats.argtypes = [vp, vp, ci]
    L.sas_read_projection.argtypes = [vp, vp, vp, vp, vp, vp]
    L.sas_read_tile_lists.argtypes = [vp, vp, vp, i64]
    L.sas_version.restype = ctypes.c_char_p
    for name in EXPORTS:
        if name not in ("sas_last_error", "sas_version"):
            getattr(L, name).restype = ci
    _lib = L
    return L


def check(ctx, rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().sas_last_error(ctx).decode() if ctx else ""
        raise SasError(f"{what} failed (status {rc}): {msg}")
