"""Object wrapper over the C ABI: one ``Rasterizer`` = one ``sas_ctx`` on one GPU.

PyTorch is plumbing here (device memory for the outputs, the current HIP stream); all
arithmetic of the frame happens in libsas_hip.so.
"""
from __future__ import annotations

import ctypes
import functools
import math
import threading
from typing import Dict, Iterable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi
from ._capi import SasError

ArrayLike = Union[np.ndarray, torch.Tensor]


def _host(a):
    """A torch tensor as a detached host NumPy array; anything else as it is."""
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def _wait_for(*inputs) -> None:
    """Device-resident torch inputs must be complete before the library copies them."""
    for a in inputs:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            torch.cuda.synchronize(a.device)


def _addr(a):
    """The address of a device tensor or a NumPy array for the C ABI; None for None and for an empty one."""
    if isinstance(a, torch.Tensor):
        return a.data_ptr() if a.numel() else None
    return a.ctypes.data if a is not None and a.size else None


def _as_f32(a: ArrayLike, shape: Tuple[int, ...], name: str):
    """Return (keepalive, pointer) of a contiguous float32 array with the given shape."""
    if isinstance(a, torch.Tensor):
        t = a.detach()
        if t.dtype != torch.float32:
            t = t.float()
        t = t.reshape(shape).contiguous()
        return t, ctypes.c_void_p(t.data_ptr())
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(shape)
    return arr, arr.ctypes.data_as(ctypes.c_void_p)


def cov3x3_to_cov6(cov: ArrayLike) -> ArrayLike:
    """[n,3,3] symmetric -> [n,6] (xx xy xz yy yz zz), the viser `covariances` argument (Door B)."""
    if isinstance(cov, torch.Tensor):
        c = cov.reshape(-1, 3, 3)
        return torch.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], dim=1).contiguous()
    c = np.asarray(cov, dtype=np.float32).reshape(-1, 3, 3)
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], axis=1)


MAX_FEATURES = 256   # channels of a feature store (sas_scene_features)
MESH_QUERY_CHUNK = _capi.SAS_QUERY_CHUNK   # triangles query_meshes' kernel stages at a time: mesh sizes around it take its chunk edges
MAX_QUERY_MESHES = 256
MATCH_CHUNK = _capi.SAS_MATCH_CHUNK   # targets match_points' kernel stages at a time: target sizes around it take its chunk edges
MATCH_MOMENTS = 18
CLOUD_RESIDENT = _capi.SAS_CLOUD_RESIDENT   # survivors per cloud sample_point_cloud's sampling kernel keeps in registers: beyond it they stream
LIFT_ONE = _capi.SAS_LIFT_ONE   # 2**32: the fixed-point unit of lift_labels' votes (a weight of 1.0)
LIFT_FEATURE_ONE = _capi.SAS_LIFT_FEATURE_ONE   # 2**24: the fixed-point unit of lift_features' weights


def _views_and_frame(viewmats, frame):
    """``viewmats [C,4,4]`` and ``frame`` (4x4, or None) as float64 arrays; ValueError on a wrong shape."""
    V = np.asarray(_host(viewmats), dtype=np.float64)
    if V.ndim != 3 or V.shape[1:] != (4, 4):
        raise ValueError(f"viewmats must be [C,4,4], got {list(V.shape)}")
    F = None if frame is None else np.asarray(_host(frame), dtype=np.float64)
    if F is not None and F.shape != (4, 4):
        raise ValueError(f"frame must be 4x4, got {list(F.shape)}")
    return V, F


def cloud_transforms(viewmats, frame=None) -> np.ndarray:
    """Camera-to-output-frame maps of ``sample_point_cloud``: ``[C,12]`` float32 rows ``A|t``, the rigid inverse of every world-to-camera
    ``viewmats [C,4,4]`` (``R^T | -R^T t``, in float64) with ``frame`` (4x4, world to output frame; any affine map) multiplied on from
    the left, rounded to float32 once.  ValueError on a wrong shape."""
    V, F = _views_and_frame(viewmats, frame)
    inv = np.zeros_like(V)
    Rt = np.transpose(V[:, :3, :3], (0, 2, 1))
    inv[:, :3, :3] = Rt
    inv[:, :3, 3] = -np.einsum("cij,cj->ci", Rt, V[:, :3, 3])
    inv[:, 3, 3] = 1.0
    if F is not None:
        inv = F[None] @ inv
    return np.ascontiguousarray(inv[:, :3, :].reshape(-1, 12).astype(np.float32))


def fuse_transforms(viewmats, frame=None) -> np.ndarray:
    """Volume-frame-to-camera maps of ``fuse_depth``: ``[C,12]`` float32 rows ``A|t``, every world-to-camera ``viewmats [C,4,4]`` with
    the inverse of ``frame`` (4x4, world to volume frame; any invertible affine map -- ``cloud_transforms``' argument) multiplied on
    from the right, ``viewmat @ inv(frame)`` in float64, rounded to float32 once.  ValueError on a wrong shape."""
    V, F = _views_and_frame(viewmats, frame)
    if F is not None:
        V = V @ np.linalg.inv(F)[None]
    return np.ascontiguousarray(V[:, :3, :].reshape(-1, 12).astype(np.float32))


def cloud_keep_table(keep_labels) -> Optional[np.ndarray]:
    """The 256-byte keep table of ``sample_point_cloud`` from the labels to keep (integers in 0..255); None stays None."""
    if keep_labels is None:
        return None
    ids = np.asarray(list(keep_labels), dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() > 255):
        raise ValueError("keep_labels must be labels in 0..255")
    table = np.zeros(256, np.uint8)
    table[ids] = 1
    return table


def cloud_bounds(bounds) -> Optional[np.ndarray]:
    """``bounds`` ((lo[3], hi[3]) or [2,3] / [6]) as the float32 ``lo, hi`` row of ``sample_point_cloud``; None stays None."""
    if bounds is None:
        return None
    b = np.asarray(_host(bounds), dtype=np.float32)
    if b.size != 6:
        raise ValueError(f"bounds must be (lo[3], hi[3]), got shape {list(b.shape)}")
    return np.ascontiguousarray(b.reshape(6))


def pack_query_meshes(meshes) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``[(vertices [V,3], faces [F,3]), ...]`` as one call's arrays (sas_query_meshes): vertices float32 (rounded once), faces int32
    re-based into the joint vertex array, triangle offsets int64 ``[M+1]``.  ValueError on a face index outside its own mesh."""
    if not 1 <= len(meshes) <= MAX_QUERY_MESHES:
        raise ValueError(f"query_meshes takes 1..{MAX_QUERY_MESHES} meshes, got {len(meshes)}")
    vs, fs, offsets, base = [], [], [0], 0
    for k, (v, f) in enumerate(meshes):
        v = np.asarray(_host(v), dtype=np.float64).reshape(-1, 3).astype(np.float32)
        f = np.asarray(_host(f), dtype=np.int64).reshape(-1, 3)
        if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
            raise ValueError(f"mesh {k}: face indices out of [0,{v.shape[0]})")
        vs.append(v)
        fs.append(f + base)
        base += v.shape[0]
        offsets.append(offsets[-1] + f.shape[0])
    return (np.ascontiguousarray(np.concatenate(vs)), np.ascontiguousarray(np.concatenate(fs).astype(np.int32)),
            np.asarray(offsets, dtype=np.int64))


def feature_channels(shape: Sequence[int], n: int) -> int:
    """Channels C of a feature array of ``shape`` for a scene of ``n`` Gaussians ([n,C], 1 <= C <= 256); ValueError otherwise."""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 2 or shape[0] != n:
        raise ValueError(f"features must be [N={n},C], got {list(shape)}")
    if not 1 <= shape[1] <= MAX_FEATURES:
        raise ValueError(f"features must have 1..{MAX_FEATURES} channels, got {shape[1]}")
    return shape[1]


def _mesh_features_sit_beside(n_triangles: int, channels: int) -> None:
    """Mesh features sit beside meshes and a feature store: ValueError without either."""
    if n_triangles <= 0:
        raise ValueError("mesh features need meshes (upload_meshes)")
    if channels <= 0:
        raise ValueError("mesh features need a feature store (upload_features)")


def mesh_feature_channels(shape: Sequence[int], n_triangles: int, channels: int) -> int:
    """Channels of a per-triangle feature array of ``shape`` for meshes of ``n_triangles`` triangles beside a feature store of
    ``channels`` channels ([T,C] with C the store's); ValueError otherwise."""
    _mesh_features_sit_beside(n_triangles, channels)
    shape = tuple(int(v) for v in shape)
    if len(shape) != 2 or shape[0] != n_triangles:
        raise ValueError(f"mesh features must be [T={n_triangles},C], got {list(shape)}")
    if shape[1] != channels:
        raise ValueError(f"mesh features must have the feature store's {channels} channels, got {shape[1]}")
    return shape[1]


def mesh_onehot_channels(groups: np.ndarray, n_triangles: int, channels: int) -> int:
    """Channels of the one-hot mesh features (a triangle's pose group is its channel) beside a feature store of ``channels``
    channels: every triangle's group must have a channel; ValueError otherwise."""
    _mesh_features_sit_beside(n_triangles, channels)
    g = np.asarray(groups).reshape(-1)
    if g.shape[0] != n_triangles:
        raise ValueError(f"{g.shape[0]} mesh groups for {n_triangles} triangles")
    if g.size and int(g.max()) >= channels:
        raise ValueError(f"one-hot mesh features: pose group {int(g.max())} has no channel among {channels}")
    return channels


def feature_background_array(fbg, C: int) -> Optional[np.ndarray]:
    """The feature background as a float32 host array [C] (None: zeros, passed as NULL); ValueError on a wrong length."""
    if fbg is None:
        return None
    a = np.ascontiguousarray(np.asarray(_host(fbg), dtype=np.float32)).reshape(-1)
    if a.shape[0] != C:
        raise ValueError(f"feature_background must have {C} values, got {a.shape[0]}")
    return a


def group_labels(weights: torch.Tensor, alpha: torch.Tensor, min_alpha: float = 0.5) -> torch.Tensor:
    """Per-pixel splat group of group weights [H,W,G] (render_group_masks): the argmax over groups, ties to the lowest
    group id, and 255 where ``alpha [H,W,1] < min_alpha``.  uint8 [H,W] (with 256 groups, group 255 reads as none)."""
    G = int(weights.shape[-1])
    top = weights.max(dim=-1, keepdim=True).values
    ids = torch.arange(G, dtype=torch.int32, device=weights.device)
    lab = torch.where(weights == top, ids, torch.full_like(ids, G)).min(dim=-1).values.clamp_(max=255)
    lab = torch.where(alpha[..., 0] < min_alpha, torch.full_like(lab, 255), lab)
    return lab.to(torch.uint8)


_ASYNC, _FILL, _MESH_SURFACE, _FAST_EXP, _TIMING, _FULL_SORT, _TIME_TILES = (
    _capi.SAS_ASYNC, _capi.SAS_DEPTH_FILL_MAX, _capi.SAS_MESH_SURFACE, _capi.SAS_FAST_EXP, _capi.SAS_TIMING, _capi.SAS_FULL_SORT, _capi.SAS_TIME_TILES)


def _flags(block=True, depth_fill_max=False, mesh_surface=False, fast_exp=False, timing=False, full_sort=False, time_tiles=False) -> int:
    """The flags word of a render call (SAS_* of include/sim_a_splat_amd.h); module constants, called by position: render's path."""
    return (0 if block else _ASYNC) | (_FILL if depth_fill_max else 0) | (_MESH_SURFACE if mesh_surface else 0) | \
           (_FAST_EXP if fast_exp else 0) | (_TIMING if timing else 0) | (_FULL_SORT if full_sort else 0) | (_TIME_TILES if time_tiles else 0)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # (private, but what torch.cuda.current_stream itself calls)


def _locked(fn):
    """One caller at a time per context: the C ABI is not re-entrant (include/sim_a_splat_amd.h), and the reference's
    callers are not always single-threaded -- demo_hw_splat.py drives env.step from a ROS2 callback thread
    (examples/demo_hw_splat.py:113-136) while a viewer thread may render through the same scene."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        with self._lock:
            return fn(self, *args, **kwargs)
    return wrapper


class Rasterizer:
    """MI355X Gaussian-splat rasterizer context (HIP, gfx950).  Every method that enters the C ABI holds the
    context's lock (re-entrant: a thread may nest calls)."""

    def __init__(self, device: Union[int, str, torch.device] = 0):
        if not torch.cuda.is_available():
            raise SasError("no HIP device visible: the render path has no CPU fallback")
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if dev.type != "cuda":
            raise SasError(f"Rasterizer needs a cuda (HIP) device, got {dev}")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._dev_index = int(self.device.index)
        self._lock = threading.RLock()
        self._L = _capi.lib()
        self._ctx = ctypes.c_void_p()
        rc = self._L.sas_create(self.device.index, ctypes.byref(self._ctx))
        if rc != 0:
            raise SasError(f"sas_create(device={self.device.index}) failed with status {rc}")
        self.n = 0
        self.n_groups = 0
        self.sh_degree, self.covariance_form = 3, "quats"   # of the scene last uploaded (render_backward shapes its outputs by them)
        self._group_ids = None
        self._forget("scene")
        self._keep = []  # outputs of in-flight async frames (the C ABI keeps up to four)
        self._argcache = {}  # id(argument) -> (argument, float32 array, address): _host_arg

    # -- lifetime ---------------------------------------------------------------------------
    @_locked
    def close(self) -> None:
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._L.sas_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str) -> None:
        _capi.check(self._ctx, rc, what)

    def _forget(self, *stores: str) -> None:
        """Reset what this object remembers of the library's stores, by the library's rule (sas_api.cpp: forget): features and meshes sit
        beside a scene, mesh features beside both.  The only place these fields are reset; each ``upload*`` sets its own in one line."""
        s = set(stores)
        if "scene" in s:
            s |= {"features", "meshes"}
            self._skin_k = 0       # entries per Gaussian of the bound skin (set_skin; 0: none): a new scene has none
            self._deform_m = 0     # nodes of the last deform since the bind (0: none): deform_backward's row count
        if s & {"features", "meshes"}:
            s.add("mesh_features")
        if "meshes" in s:          # vertex attributes sit beside the meshes (upload_mesh_vertex_attributes)
            s.add("mesh_attributes")
        if "features" in s:        # channels of the feature store (upload_features; 0: none for this scene); it is the groups' one-hot
            self.n_features, self._features_onehot = 0, False
        if "meshes" in s:          # triangles of the meshes (upload_meshes; 0: none for this scene), their pose groups
            self.n_mesh_triangles, self.n_mesh_vertices, self._mesh_groups = 0, 0, np.zeros(0, np.uint8)
        if "mesh_attributes" in s:   # the meshes carry vertex normals and / or colours (smooth shading, rule 2b)
            self.mesh_vertex_attributes = False
        if "mesh_features" in s:   # the meshes' feature rows are the one-hot of the triangles' pose groups (upload_mesh_features)
            self._mesh_features_onehot = False

    def _store_rows(self, entry: str, rows: Optional[ArrayLike], count: int, C: int, name: str) -> None:
        """``rows [count,C]`` (None: one-hot, built on the device) into the feature store that C-ABI ``entry`` fills."""
        pf = None
        if rows is not None:
            f, pf = _as_f32(rows, (count, C), name)
            _wait_for(f)
        self._check(getattr(self._L, entry)(self._ctx, count, C, pf), entry)

    # -- scene ------------------------------------------------------------------------------
    @_locked
    def upload(self, means: ArrayLike, opacities: ArrayLike, colors: ArrayLike, *, quats: Optional[ArrayLike] = None,
               scales: Optional[ArrayLike] = None, covariances: Optional[ArrayLike] = None, sh_degree: int = 3,
               group_id: Optional[ArrayLike] = None, n_groups: int = 0) -> None:
        """Replace the scene.  ``sh_degree < 0``: ``colors`` is final RGB [n,3] (Door B)."""
        n = int(means.shape[0])
        keep = []
        m, pm = _as_f32(means, (n, 3), "means"); keep.append(m)
        o, po = _as_f32(opacities, (n,), "opacities"); keep.append(o)
        kk = (sh_degree + 1) ** 2 if sh_degree >= 0 else 1
        c, pc = _as_f32(colors, (n, kk, 3), "colors"); keep.append(c)
        pq = ps = pcov = None
        if quats is not None and scales is not None:
            q, pq = _as_f32(quats, (n, 4), "quats"); keep.append(q)
            s, ps = _as_f32(scales, (n, 3), "scales"); keep.append(s)
        elif covariances is not None:
            cov = covariances
            if tuple(cov.shape[1:]) == (3, 3):
                cov = cov3x3_to_cov6(cov)
            cv, pcov = _as_f32(cov, (n, 6), "covariances"); keep.append(cv)
        else:
            raise ValueError("need quats+scales or covariances")
        pg = None
        if group_id is not None:
            if isinstance(group_id, torch.Tensor):
                g = group_id.detach().to(torch.uint8).contiguous()
                pg = ctypes.c_void_p(g.data_ptr())
            else:
                g = np.ascontiguousarray(np.asarray(group_id, dtype=np.uint8))
                pg = g.ctypes.data_as(ctypes.c_void_p)
            keep.append(g)
            if n_groups <= 0:
                n_groups = int(g.max()) + 1 if n > 0 else 1
        torch.cuda.synchronize(self.device)  # device-resident inputs must be complete before the copy
        self._check(self._L.sas_scene_upload(self._ctx, n, pm, pq, ps, pcov, po, pc, int(sh_degree), pg, int(n_groups)),
                    "sas_scene_upload")
        self.n = n
        self.n_groups = int(n_groups) if group_id is not None else 0
        self.sh_degree, self.covariance_form = int(sh_degree), "quats" if pq is not None else "cov6"
        self._group_ids = g if group_id is not None else None   # (bind_skin(group=...) selects by them)
        self._forget("scene")

    @_locked
    def upload_features(self, features: Optional[ArrayLike] = None) -> None:
        """Per-Gaussian feature channels for ``render_features``: ``[N,C]`` numpy or torch (host or device, the order of
        ``upload``), 1 <= C <= 256; NaN and +-Inf are mapped to -+FLT_MAX as colours are.  ``None``: one-hot of the scene's
        splat groups (C = n_groups), built on the device.  A new ``upload`` forgets them.  Mesh features
        (``upload_mesh_features``) belong to the store they were set beside: this call forgets them."""
        self._forget("mesh_features")
        if features is None and self.n_groups <= 0:
            raise ValueError("one-hot group features need a scene uploaded with group_id")
        C = self.n_groups if features is None else feature_channels(features.shape, self.n)
        self._store_rows("sas_scene_features", features, self.n, C, "features")
        self.n_features, self._features_onehot = C, features is None

    @_locked
    def upload_meshes(self, vertices: ArrayLike, triangles: ArrayLike, colors: ArrayLike, groups: Optional[ArrayLike] = None,
                      ambient: float = 0.4, diffuse: float = 0.6, vertex_normals: Optional[ArrayLike] = None,
                      vertex_colors: Optional[ArrayLike] = None) -> None:
        """Triangle meshes composited into every frame (sas_scene_meshes; DESIGN.md 3, "Meshes"): ``vertices [V,3]`` (mesh-local,
        scale applied), ``triangles [T,3]`` vertex indices, ``colors [T,3]`` (or one ``[3]`` for all), ``groups [T]`` the pose
        group moving each triangle (``None``: group 0).  Shading ``clamp(c (ambient + diffuse |n . v|), 0, 1)``.  Frames then take
        the full-sort path.  A new ``upload`` forgets the meshes; ``T == 0`` clears them.  Mesh features
        (``upload_mesh_features``) and vertex attributes are forgotten; ``vertex_normals`` / ``vertex_colors`` ``[V,3]`` are then
        handed to ``upload_mesh_vertex_attributes`` (smooth shading)."""
        self._forget("mesh_features", "mesh_attributes")
        v = np.ascontiguousarray(np.asarray(_host(vertices), dtype=np.float32).reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(_host(triangles), dtype=np.int64).reshape(-1, 3))
        if t.size and (t.min() < 0 or t.max() >= v.shape[0]):
            raise ValueError(f"triangle indices out of [0,{v.shape[0]})")
        t = np.ascontiguousarray(t.astype(np.int32))
        T = t.shape[0]
        c = np.asarray(_host(colors), dtype=np.float32)
        c = np.ascontiguousarray(np.broadcast_to(c.reshape(-1, 3) if c.size != 3 else c.reshape(1, 3), (T, 3)))
        g = np.zeros(T, np.uint8) if groups is None else np.asarray(_host(groups))
        if g.size and (g.min() < 0 or g.max() > 255):
            raise ValueError("mesh groups must be in [0,255]")
        g = np.ascontiguousarray(np.broadcast_to(g.astype(np.uint8).reshape(-1), (T,)))
        self._check(self._L.sas_scene_meshes(self._ctx, v.shape[0], v.ctypes.data, T, t.ctypes.data, c.ctypes.data, g.ctypes.data,
                                             float(ambient), float(diffuse)), "sas_scene_meshes")
        self.n_mesh_triangles, self.n_mesh_vertices, self._mesh_groups = T, v.shape[0], g
        if T and (vertex_normals is not None or vertex_colors is not None):
            self.upload_mesh_vertex_attributes(vertex_normals, vertex_colors)

    @_locked
    def upload_mesh_vertex_attributes(self, normals: Optional[ArrayLike] = None, colors: Optional[ArrayLike] = None) -> None:
        """Vertex attributes of the uploaded meshes (sas_scene_mesh_vertex_attributes; DESIGN.md 3, "Meshes", rule 2b):
        ``normals [V,3]`` unit, mesh-local (zero or non-finite: the vertex has none) and / or ``colors [V,3]`` in [0,1], V the
        vertex count of ``upload_meshes``.  A triangle whose three vertices have a normal is shaded smoothly -- the headlight
        shade evaluated per vertex and interpolated perspective-correctly over the triangle; the others stay flat.  Without
        ``colors`` a smooth triangle keeps its own colour.  Both ``None`` clears the attributes; ``upload`` and
        ``upload_meshes`` forget them."""
        arr = lambda a: None if a is None else np.ascontiguousarray(np.asarray(_host(a), dtype=np.float32).reshape(-1, 3))
        n, c = arr(normals), arr(colors)
        count = next((a.shape[0] for a in (n, c) if a is not None), self.n_mesh_vertices)
        if n is not None and c is not None and n.shape[0] != c.shape[0]:
            raise ValueError(f"{n.shape[0]} vertex normals, {c.shape[0]} vertex colours")
        self._check(self._L.sas_scene_mesh_vertex_attributes(self._ctx, count, None if n is None else n.ctypes.data,
                                                             None if c is None else c.ctypes.data), "sas_scene_mesh_vertex_attributes")
        self.mesh_vertex_attributes = n is not None or c is not None

    @_locked
    def clear_meshes(self) -> None:
        self._forget("mesh_features")
        self._check(self._L.sas_scene_meshes(self._ctx, 0, None, 0, None, None, None, 0.4, 0.6), "sas_scene_meshes")
        self._forget("meshes")

    @_locked
    def upload_mesh_features(self, features: Optional[ArrayLike] = None) -> None:
        """Per-triangle feature rows for ``render_features`` of a scene with meshes (sas_scene_mesh_features): ``[T,C]`` numpy
        or torch, the triangle order of ``upload_meshes``, C the channels of ``upload_features``; taken as they are (not
        shaded), NaN and +-Inf mapped as colours are.  ``None``: one-hot of each triangle's pose group.  Where a pixel
        shows a triangle its row takes the feature background's place.  ``upload``, ``upload_meshes`` and
        ``upload_features`` forget them -- and ``render_features`` refuses a scene with meshes until they are set."""
        T = self.n_mesh_triangles
        C = mesh_onehot_channels(self._mesh_groups, T, self.n_features) if features is None else mesh_feature_channels(features.shape, T, self.n_features)
        self._store_rows("sas_scene_mesh_features", features, T, C, "mesh features")
        self._mesh_features_onehot = features is None

    # -- queries ----------------------------------------------------------------------------
    @_locked
    def query_meshes(self, points: ArrayLike, meshes, max_distance: float = float("inf")) -> Dict[str, torch.Tensor]:
        """Distance and inside test of ``points [N,3]`` against ``meshes``, a list of ``(vertices [V,3], faces [F,3])`` already in
        the points' frame (sas_query_meshes; DESIGN.md 3, "Mesh queries").  Returns float32 device tensors ``[M,N]``:
        ``distance``, the unsigned Euclidean distance to mesh m, and ``winding``, its generalised winding number (1 inside a closed,
        outward-oriented mesh, 0 outside).  A pair whose point lies outside the mesh's box inflated by ``max_distance`` is culled
        and reads ``+inf`` / ``0``, as does a point with a non-finite coordinate; ``inf`` culls nothing else.  Needs no scene and
        leaves the uploaded one alone."""
        v, f, offsets = pack_query_meshes(meshes)
        n = int(points.shape[0])
        p, pp = _as_f32(points, (n, 3), "points")
        _wait_for(p)
        M = len(offsets) - 1
        res = {k: torch.empty((M, n), dtype=torch.float32, device=self.device) for k in ("distance", "winding")}
        if n == 0:
            return res
        self._check(self._L.sas_query_meshes(self._ctx, n, pp, v.shape[0], v.ctypes.data, f.shape[0], f.ctypes.data, M,
                                             offsets.ctypes.data, float(max_distance), res["distance"].data_ptr(), res["winding"].data_ptr(),
                                             self._stream()), "sas_query_meshes")
        return res

    @_locked
    def match_points(self, source: ArrayLike, target: ArrayLike, transform=None, max_distance: float = float("inf"),
                     slices: Optional[int] = None) -> Dict[str, object]:
        """For every point of ``source [S,3]`` moved by ``transform`` (4x4 or 3x4, rounded to float32; None: the identity) the
        nearest point of ``target [T,3]`` within ``max_distance`` (sas_match_points; DESIGN.md 3, "Point matching").  Returns
        ``index`` (int32 ``[S]``, -1 without a match) and ``dist2`` (float32 ``[S]``, +inf without one) as device tensors, and
        ``moments``, a float64 ndarray of 18 over the held matches: n, sum p' (3), sum q (3), sum q p'^T (9), sum |p'|^2, sum d2.
        Ties go to the lowest target index.  Torch device tensors are read where they are: an ICP loop keeps both clouds on the
        device.  ``slices``: None is the library's choice; no result depends on it.  Needs no scene."""
        ns, nt = int(source.shape[0]), int(target.shape[0])
        s, sp = _as_f32(source, (ns, 3), "source")
        t, tp = _as_f32(target, (nt, 3), "target")
        _wait_for(s, t)
        A = None
        if transform is not None:
            A = np.asarray(_host(transform), dtype=np.float64)
            if A.shape not in ((4, 4), (3, 4)):
                raise ValueError(f"transform must be 4x4 or 3x4, got {list(A.shape)}")
            A = np.ascontiguousarray(A[:3].astype(np.float32)).reshape(12)
        index = torch.full((ns,), -1, dtype=torch.int32, device=self.device)
        dist2 = torch.full((ns,), float("inf"), dtype=torch.float32, device=self.device)
        moments = np.zeros(MATCH_MOMENTS, np.float64)
        self._check(self._L.sas_match_points(self._ctx, ns, sp, nt, tp, A.ctypes.data if A is not None else None, float(max_distance),
                                             0 if slices is None else int(slices), index.data_ptr() if ns else None,
                                             dist2.data_ptr() if ns else None, moments.ctypes.data, self._stream()), "sas_match_points")
        return {"index": index, "dist2": dist2, "moments": moments}

    def _device_image(self, a, dtype, count: int, name: str, shape) -> torch.Tensor:
        """A per-pixel input of ``sample_point_cloud`` on this context's device: a device tensor of the right type as it is (read in
        place), anything else converted and copied."""
        if isinstance(a, torch.Tensor):
            t = a.detach().to(device=self.device, dtype=dtype).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype={torch.float32: np.float32, torch.uint8: np.uint8}[dtype]))).to(self.device)
        if t.numel() != count:
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
        return t

    def _depth_views(self, C: int, W: int, H: int, depth, Ks, rgb8, labels, keep_labels):
        """What ``sample_point_cloud`` and ``fuse_depth`` make of their views' inputs: ``Ks [C,3,3]`` as 9 C float32 on the host, the keep
        table of ``keep_labels`` (which need ``labels``), and ``depth``, ``rgb8``, ``labels`` on the device (None stays None)."""
        Kc = np.ascontiguousarray(np.asarray(_host(Ks), dtype=np.float32)).reshape(-1)
        if Kc.size != 9 * C:
            raise ValueError(f"Ks must be [{C},3,3], got {Kc.size} values")
        if keep_labels is not None and labels is None:
            raise ValueError("keep_labels needs labels")
        keep = cloud_keep_table(keep_labels)
        d = self._device_image(depth, torch.float32, C * H * W, "depth", (C, H, W))
        c8 = None if rgb8 is None else self._device_image(rgb8, torch.uint8, 3 * C * H * W, "rgb8", (C, H, W, 3))
        lab = None if labels is None else self._device_image(labels, torch.uint8, C * H * W, "labels", (C, H, W))
        return Kc, keep, d, c8, lab

    def _blocking_call(self, entry: str, *args) -> None:
        """C-ABI ``entry(ctx, *args, stream)``, blocking, on the caller's stream: it runs behind what the stream holds (``_device_image``'s copies)."""
        rc = getattr(self._L, entry)(self._ctx, *args, self._stream())
        if rc != 0:
            self._check(rc, entry)
        self._in_flight(True)

    @_locked
    def sample_point_cloud(self, depth: ArrayLike, viewmats: ArrayLike, Ks: ArrayLike, width: int, height: int, n_points: int, *,
                           rgb8: Optional[ArrayLike] = None, labels: Optional[ArrayLike] = None, keep_labels=None, bounds=None,
                           voxel_size: float = 0.0, stride: int = 1, frame=None, clouds: Optional[Sequence[int]] = None,
                           n_clouds: int = 1, timing: bool = False) -> Dict[str, torch.Tensor]:
        """Fixed-size point clouds from the depth frames of C same-sized views (sas_sample_points; DESIGN.md 3, "Point clouds"):
        ``depth [C,H,W]`` (or ``[C,H,W,1]``) float32 with ``viewmats [C,4,4]`` (world to camera) and ``Ks [C,3,3]``, optionally
        ``rgb8 [C,H,W,3]`` and ``labels [C,H,W]`` uint8 -- device tensors are read where they are (the outputs of
        ``render_batch_labels``), NumPy arrays are copied.  Every pixel with a depth in (0, inf) is unprojected and moved by
        ``cloud_transforms(viewmats, frame)`` -- into the world, or with ``frame`` (4x4, world to output frame) beyond it --
        kept if it lies within ``bounds`` ``(lo[3], hi[3])`` (inclusive) and, with ``labels`` and ``keep_labels`` (the labels to
        keep), shows one of them; ``stride`` looks at every stride-th row and column only; ``voxel_size > 0`` keeps one point (the
        lowest pixel index) per cell of a grid over ``bounds``.  View v feeds cloud ``clouds[v]`` of ``n_clouds`` (None: all feed
        cloud 0).  Each cloud is cut to ``n_points`` by farthest-point sampling from its first survivor.  Returns device tensors
        in pick order: ``points [E,K,3]`` float32, ``index [E,K]`` int32 (the flat pixel ``(c H + v) W + u``; -1 padding),
        ``count [E]`` int32 (survivors before sampling) and, with the inputs, ``colors [E,K,3]`` uint8 and ``labels [E,K]`` uint8
        (255 padding).  Deterministic; blocking; needs no scene.  ``timing``: ``stage_times()`` then holds the call's kernels
        (project: marking, scatter: compaction, blend: sampling)."""
        T = cloud_transforms(viewmats, frame)
        C, W, H, K, E = T.shape[0], int(width), int(height), int(n_points), int(n_clouds)
        if K < 0 or E < 1 or W < 0 or H < 0:
            raise ValueError(f"sample_point_cloud: n_points {K}, n_clouds {E}, size {W}x{H}")
        Kc, keep, d, c8, lab = self._depth_views(C, W, H, depth, Ks, rgb8, labels, keep_labels)
        b = cloud_bounds(bounds)
        cl = None
        if clouds is not None:
            cl = np.ascontiguousarray(np.asarray(clouds, dtype=np.int32).reshape(-1))
            if cl.shape[0] != C:
                raise ValueError(f"clouds must name one cloud per view ({C}), got {cl.shape[0]}")
        dev = self.device
        res = {"points": torch.empty((E, K, 3), dtype=torch.float32, device=dev), "index": torch.empty((E, K), dtype=torch.int32, device=dev),
               "count": torch.empty((E,), dtype=torch.int32, device=dev)}
        if c8 is not None:
            res["colors"] = torch.empty((E, K, 3), dtype=torch.uint8, device=dev)
        if lab is not None:
            res["labels"] = torch.empty((E, K), dtype=torch.uint8, device=dev)
        self._blocking_call("sas_sample_points", C, W, H, _addr(d), _addr(c8), _addr(lab), _addr(Kc), _addr(T), _addr(cl), E, _addr(keep), _addr(b),
                            float(voxel_size), int(stride), K, _capi.SAS_TIMING if timing else 0, _addr(res["points"]), _addr(res["index"]),
                            _addr(res.get("colors")), _addr(res.get("labels")), res["count"].data_ptr())
        return res

    @_locked
    def fuse_depth(self, volume, depth: ArrayLike, viewmats: ArrayLike, Ks: ArrayLike, width: int, height: int, *,
                   rgb8: Optional[ArrayLike] = None, labels: Optional[ArrayLike] = None, keep_labels=None, frame=None,
                   trunc: Optional[float] = None, near: float = 0.01, pixel_centre: float = 0.5, max_weight: float = 64.0,
                   timing: bool = False) -> None:
        """Integrate the depth frames of C same-sized views into ``volume`` (sas_fuse_depth; DESIGN.md 3, "Depth fusion"), in view
        order.  ``volume`` (``reconstruct.TsdfVolume``) owns the device tensors ``tsdf`` / ``weight [nz,ny,nx]`` and ``color
        [nz,ny,nx,3]`` (or None), updated in place, with ``lo``, ``voxel_size`` and ``dims = (nx, ny, nz)``.  ``depth [C,H,W]`` (or
        ``[C,H,W,1]``) float32 with ``viewmats [C,4,4]`` (world to camera) and ``Ks [C,3,3]``, optionally ``rgb8 [C,H,W,3]`` (needed
        when the volume has colour) and ``labels [C,H,W]`` uint8 -- device tensors are read where they are (the outputs of
        ``render_batch_labels``), NumPy arrays are copied.  The volume lives in the world or, with ``frame`` (4x4, world to volume
        frame), beyond it: ``fuse_transforms(viewmats, frame)``.  With ``labels`` and ``keep_labels`` a pixel that shows another
        label only carves free space in front of itself.  ``trunc``: the truncation distance in volume units (default 4 voxels),
        scaled by the cube root of ``|det A|`` of the first view's map into camera units; ``near``: camera units; ``pixel_centre``:
        0.5 for rendered depth, 0 for the convention of ``render_rgbd``'s points.  Deterministic; blocking; needs no scene.
        ``timing``: ``stage_times()`` then holds the call's kernel (blend, total)."""
        T = fuse_transforms(viewmats, frame)
        C, W, H = T.shape[0], int(width), int(height)
        if W < 0 or H < 0:
            raise ValueError(f"fuse_depth: size {W}x{H}")
        Kc, keep, d, c8, lab = self._depth_views(C, W, H, depth, Ks, rgb8, labels, keep_labels)
        nx, ny, nz = (int(n) for n in volume.dims)
        for name, t, shape in (("tsdf", volume.tsdf, (nz, ny, nx)), ("weight", volume.weight, (nz, ny, nx)), ("color", volume.color, (nz, ny, nx, 3))):
            if t is None and name == "color":
                continue
            if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"volume.{name} must be a contiguous float32 tensor {list(shape)} on {self.device}")
        if volume.color is not None and rgb8 is None:
            raise ValueError("a volume with colour needs rgb8")
        voxel = float(volume.voxel_size)
        scale = 1.0
        if C > 0:
            A = np.asarray(_host(viewmats), dtype=np.float64)[0, :3, :3]
            if frame is not None:
                A = A @ np.linalg.inv(np.asarray(_host(frame), dtype=np.float64))[:3, :3]
            scale = float(np.cbrt(abs(np.linalg.det(A))))
        tr = (4.0 * voxel if trunc is None else float(trunc)) * scale
        lo = np.ascontiguousarray(np.asarray(_host(volume.lo), dtype=np.float32).reshape(3))
        dims = np.array([nx, ny, nz], np.int32)
        self._blocking_call("sas_fuse_depth", C, W, H, _addr(d), _addr(c8), _addr(lab), _addr(Kc), _addr(T), _addr(keep), lo.ctypes.data, voxel,
                            dims.ctypes.data, tr, float(near), float(pixel_centre), float(max_weight), _capi.SAS_TIMING if timing else 0,
                            _addr(volume.tsdf), _addr(volume.weight), _addr(volume.color) if c8 is not None else None)

    @_locked
    def set_group_poses(self, Rt: ArrayLike) -> None:
        """[G,12] (or [G,3,4]) row-major (R|t) per splat group: the poses of the frames submitted from now on
        (frames in flight keep the poses they were submitted with; nothing is waited for)."""
        arr = np.ascontiguousarray(np.asarray(_host(Rt), dtype=np.float32)).reshape(-1, 12)
        self._check(self._L.sas_set_group_poses(self._ctx, arr.shape[0], arr.ctypes.data_as(ctypes.c_void_p)),
                    "sas_set_group_poses")

    @_locked
    def set_link_constants(self, scale: float, Ri, ti, Rfk, tfk, weld=None, groups=None) -> None:
        """Constants of the per-link pose algebra (sas_set_link_constants): ICP similarity ``(scale, Ri [3,3], ti [3])``,
        per-link mask-time forward kinematics ``Rfk [K,3,3]``, ``tfk [K,3]``, weld translation, the group each link drives."""
        f64 = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
        Rfk = f64(Rfk, (-1, 9))
        K = Rfk.shape[0]
        Ri, ti, tfk = f64(Ri, (9,)), f64(ti, (3,)), f64(tfk, (K, 3))
        w = f64(weld, (3,)) if weld is not None else None
        g = np.ascontiguousarray(np.asarray(groups, dtype=np.int32).reshape(K)) if groups is not None else None
        self._check(self._L.sas_set_link_constants(self._ctx, K, float(scale), Ri.ctypes.data, ti.ctypes.data, Rfk.ctypes.data,
                                                   tfk.ctypes.data, w.ctypes.data if w is not None else None,
                                                   g.ctypes.data if g is not None else None), "sas_set_link_constants")

    @_locked
    def set_link_poses(self, q_msg, p_msg, out: Optional[np.ndarray] = None) -> Optional[np.ndarray]:
        """A draw message's link poses (``q_msg [k,4]`` wxyz, ``p_msg [k,3]``) -> group poses, evaluated inside the
        library (sas_set_link_poses); ``out`` (float32, ``n_groups * 12`` elements) receives all current group poses."""
        q = np.ascontiguousarray(np.asarray(q_msg, dtype=np.float64).reshape(-1, 4))
        p = np.ascontiguousarray(np.asarray(p_msg, dtype=np.float64).reshape(-1, 3))
        if out is not None and not (out.dtype == np.float32 and out.flags.c_contiguous and out.size == 12 * self.n_groups):
            raise ValueError("out must be a contiguous float32 array of n_groups * 12 elements")
        rc = self._L.sas_set_link_poses(self._ctx, q.shape[0], q.ctypes.data, p.ctypes.data, out.ctypes.data if out is not None else None)
        if rc != 0:
            self._check(rc, "sas_set_link_poses")
        return out

    @_locked
    def link_attached_frame(self, q_link, p_link, local_xyz) -> Tuple[np.ndarray, np.ndarray]:
        """(wxyz, xyz) of a camera riding on a link (sas_link_attached_frame; the ICP similarity of set_link_constants)."""
        a = np.empty(17, np.float64)
        a[0:4], a[4:7], a[7:10] = q_link, p_link, local_xyz
        base = a.ctypes.data
        rc = self._L.sas_link_attached_frame(self._ctx, base, base + 32, base + 56, base + 80, base + 112)
        if rc != 0:
            self._check(rc, "sas_link_attached_frame")
        return a[10:14], a[14:17]

    @_locked
    def get_group_poses(self) -> np.ndarray:
        out = np.zeros((self.n_groups, 12), np.float32)
        self._check(self._L.sas_get_group_poses(self._ctx, self.n_groups, out.ctypes.data), "sas_get_group_poses")
        return out

    # -- frames -----------------------------------------------------------------------------
    _SHAPES = {"rgb": (3, torch.float32), "alpha": (1, torch.float32), "depth": (1, torch.float32),
               "rgb8": (3, torch.uint8)}
    _LABEL_SHAPES = dict(_SHAPES, labels=(None, torch.uint8))   # channels None: no channel axis

    @staticmethod
    def _host_f32(a, count: int) -> np.ndarray:
        a = _host(a)
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.size == count):
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(count)
        return a

    def _outputs(self, names: Iterable[str], shapes, H: int, W: int, out, views: Optional[int] = None):
        """(tensors, addresses) of the outputs ``names``, ``[H,W,channels]`` by the table ``shapes`` (``[H,W]`` where it gives no
        channels; ``[views,...]`` for a batch): ``out``'s where it holds one, validated, else allocated.  Addresses of outputs not
        asked for: None."""
        res: Dict[str, torch.Tensor] = {}
        ptrs = dict.fromkeys(shapes)
        dev = self.device
        given = out.get if out is not None else None
        for k in names:
            ch, dt = shapes[k]   # KeyError: unknown output
            shape = (H, W) if ch is None else (H, W, ch)
            if views is not None:
                shape = (views,) + shape
            t = given(k) if given else None
            if t is None:
                t = torch.empty(shape, dtype=dt, device=dev)
            elif t.shape != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"out[{k!r}] must be a contiguous {dt} tensor {shape} on {dev}")
            res[k] = t
            ptrs[k] = t.data_ptr()
        return res, ptrs

    @staticmethod
    def _host_frames(out: Optional[torch.Tensor], shape: Tuple[int, int, int, int]) -> torch.Tensor:
        """The ``[C,H,W,3]`` uint8 host tensor of the two host entry points: the caller's, validated, or a pinned one."""
        if out is None:
            return torch.empty(shape, dtype=torch.uint8, pin_memory=True)
        if out.shape != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device.type != "cpu":
            raise ValueError(f"out must be a contiguous uint8 CPU tensor {shape}")
        return out

    def _stream(self) -> int:
        """The caller's current HIP stream on this context's device (1.9 us through torch.cuda.current_stream, 0.07 us
        through the raw getter it wraps: tools/py_overhead_probe.py)."""
        if _RAW_STREAM is not None:
            return _RAW_STREAM(self._dev_index)
        return torch.cuda.current_stream(self.device).cuda_stream

    def _host_arg(self, a, count: int):
        """(float32 host array, its address) of a call argument.  A call's K, background and often its view matrix are the
        SAME objects as in the call before: the last few (object, address) pairs are remembered -- `.ctypes.data` alone
        costs 1.1 us, three of them a per cent of a blocking 1080p frame.  Only arguments that need no conversion (the
        array IS what the C side reads, so writing into it between calls stays visible) and tuples (immutable) qualify."""
        hit = self._argcache.get(id(a))
        if hit is not None and hit[0] is a:
            return hit[1], hit[2]
        arr = self._host_f32(a, count)
        ptr = arr.ctypes.data
        if arr is a or isinstance(a, tuple):
            if len(self._argcache) >= 16:
                self._argcache.clear()
            self._argcache[id(a)] = (a, arr, ptr)   # (holds `a`: its id cannot be reused while the entry lives)
        return arr, ptr

    def _views(self, viewmats, Ks, background, width, height, batch: bool):
        """The prologue of a render call: ((view, K, background) host arrays to keep alive, their three addresses, C, W, H);
        ``batch``: ``viewmats [C,4,4]`` and ``Ks [C,3,3]``, else one view."""
        C = int(viewmats.shape[0] if isinstance(viewmats, torch.Tensor) else np.asarray(viewmats).shape[0]) if batch else 1
        V, pV = self._host_arg(viewmats, 16 * C)
        Kc, pK = self._host_arg(Ks, 9 * C)
        bg, pbg = self._host_arg(background, 3)
        return (V, Kc, bg), pV, pK, pbg, C, int(width), int(height)

    def _in_flight(self, block: bool, *keep) -> None:
        """The ring of what in-flight frames read and write: cleared by a blocking call, else ``keep`` joins the last four."""
        self._keep = [] if block else (self._keep + [keep])[-4:]

    @_locked
    def render(self, viewmat: ArrayLike, K: ArrayLike, width: int, height: int,
               background: Sequence[float] = (0.0, 0.0, 0.0), *, want: Iterable[str] = ("rgb", "alpha", "depth"),
               depth_fill_max: bool = False, fast_exp: bool = False, timing: bool = False, block: bool = True,
               full_sort: bool = False, time_tiles: bool = False, mesh_surface: bool = False,
               out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Render one view; returns device tensors ``rgb [H,W,3]``, ``alpha [H,W,1]``,
        ``depth [H,W,1]`` (float32) and/or ``rgb8 [H,W,3]`` (uint8) as listed in ``want``.

        ``block=False`` only enqueues (SAS_ASYNC): up to four frames are in flight.  Frames complete in
        submission order inside later ``render*`` calls or ``wait()``; a frame's outputs may be consumed
        (and work on the current stream is ordered behind it) only once it is complete --
        ``frames_completed()`` tells how many are.  ``full_sort=True`` orders every tile list
        completely and keeps it for ``read_tile_lists`` (same image, slower).  ``mesh_surface=True`` (SAS_MESH_SURFACE):
        where a mesh triangle shows, ``alpha`` is 1 and ``depth`` closes on the triangle -- the scene's depth, not that of
        the splats in front of the mesh; rgb and every other pixel keep their bits."""
        V, pV = self._host_arg(viewmat, 16)      # _views and _in_flight written out: a method call is 0.1 - 0.2 us of this per-frame path
        Kc, pK = self._host_arg(K, 9)
        bg, pbg = self._host_arg(background, 3)
        W, H = int(width), int(height)
        res, ptrs = self._outputs(want, self._SHAPES, H, W, out)
        flags = _flags(block, depth_fill_max, mesh_surface, fast_exp, timing, full_sort, time_tiles)
        stream = self._stream()
        rc = self._L.sas_render(self._ctx, pV, pK, W, H, pbg, flags,
                                ptrs["rgb"], ptrs["alpha"], ptrs["depth"], ptrs["rgb8"], stream)
        if rc != 0:
            self._check(rc, "sas_render")
        self._keep = [] if block else (self._keep + [(res, V, Kc, bg)])[-4:]
        return res

    @_locked
    def render_rgbd(self, viewmat: ArrayLike, K: ArrayLike, width: int, height: int,
                    background: Sequence[float] = (0.0, 0.0, 0.0), *, max_depth: Optional[float] = 1.0,
                    depth_fill_max: bool = True, mesh_surface: bool = False) -> Dict[str, torch.Tensor]:
        """Render with the RGB-D consumer fused into the depth pass (sas_render_rgbd): besides
        ``rgb``/``alpha``/``depth`` returns ``points [H,W,3]`` (camera frame) and ``mask [H,W]``
        (bool, ``depth < max_depth``; all true for ``max_depth=None``) -- nerfstudio_utils.py:424-445.
        ``mesh_surface=True``: depth, points and mask include the meshes' surfaces (see ``render``)."""
        keep, pV, pK, pbg, _, W, H = self._views(viewmat, K, background, width, height, False)   # (keep: the host arrays live to the end of this blocking call)
        res = {k: torch.empty((H, W, ch), dtype=dt, device=self.device)
               for k, (ch, dt) in self._SHAPES.items() if k != "rgb8"}
        res["points"] = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        mask8 = torch.empty((H, W), dtype=torch.uint8, device=self.device)
        md = ctypes.c_float(max_depth) if max_depth is not None else None
        flags = _flags(True, depth_fill_max, mesh_surface)
        stream = self._stream()
        rc = self._L.sas_render_rgbd(self._ctx, pV, pK, W, H, pbg, flags,
                                     ctypes.addressof(md) if md is not None else None,
                                     res["rgb"].data_ptr(), res["alpha"].data_ptr(), res["depth"].data_ptr(),
                                     res["points"].data_ptr(), mask8.data_ptr(), stream)
        if rc != 0:
            self._check(rc, "sas_render_rgbd")
        self._in_flight(True)
        res["mask"] = mask8.view(torch.bool)
        return res

    @_locked
    def render_features(self, viewmat: ArrayLike, K: ArrayLike, width: int, height: int,
                        background: Sequence[float] = (0.0, 0.0, 0.0), *, feature_background=None,
                        want: Iterable[str] = ("features",), fast_exp: bool = False, depth_fill_max: bool = False,
                        block: bool = True, mesh_surface: bool = False,
                        out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Render one view with the feature channels of ``upload_features``: ``features [H,W,C]`` float32, not clamped,
        ``F = sum_i w_i f_i + (1 - alpha) feature_background`` with the frame's own weights w_i (``feature_background``:
        [C], default zeros), plus any of ``rgb`` / ``alpha`` / ``depth`` listed in ``want`` (bit-identical to ``render``).
        ``block=False`` enqueues as ``render`` does.  A scene with meshes needs ``upload_mesh_features``: the sum then
        stops at the pixel's triangle, whose row stands in ``feature_background``'s place (the ``alpha`` of that formula is
        the splats' whatever ``mesh_surface``, which only changes the alpha / depth outputs as in ``render``)."""
        C = self.n_features
        if C <= 0:
            raise SasError("render_features: no features uploaded for this scene (upload_features)")
        fb = feature_background_array(feature_background, C)
        keep, pV, pK, pbg, _, W, H = self._views(viewmat, K, background, width, height, False)
        shapes = dict(self._SHAPES, features=(C, torch.float32))
        shapes.pop("rgb8")
        want = tuple(want)
        res, ptrs = self._outputs(set(want) | {"features"}, shapes, H, W, out)
        flags = _flags(block, depth_fill_max, mesh_surface, fast_exp)
        rc = self._L.sas_render_features(self._ctx, pV, pK, W, H, pbg, fb.ctypes.data if fb is not None else None, flags,
                                         ptrs["rgb"], ptrs["alpha"], ptrs["depth"], ptrs["features"], self._stream())
        if rc != 0:
            self._check(rc, "sas_render_features")
        self._in_flight(block, res, keep, fb)
        return {k: res[k] for k in want}

    @_locked
    def render_group_masks(self, viewmat: ArrayLike, K: ArrayLike, width: int, height: int, *,
                           min_alpha: float = 0.5) -> Dict[str, torch.Tensor]:
        """Which pose group (robot link, mesh) each pixel shows: ``weights [H,W,G]`` (the one-hot group features composited, zero
        background), ``labels [H,W]`` uint8 (``group_labels``: argmax, ties to the lowest id, 255 where alpha < min_alpha)
        and ``alpha [H,W,1]``.  Selects the one-hot group store (replacing features uploaded before) for the Gaussians and,
        when the scene holds meshes, for the triangles; ``alpha`` then counts a mesh as opaque (``mesh_surface``), so that
        the weights still sum to it."""
        self._select_onehot_stores()
        o = self.render_features(viewmat, K, width, height, want=("features", "alpha"), mesh_surface=self.n_mesh_triangles > 0)
        return {"weights": o["features"], "labels": group_labels(o["features"], o["alpha"], min_alpha), "alpha": o["alpha"]}

    def _batch_call(self, name: str, C: int, pV, pK, pose_sets, pose_set, *tail) -> None:
        """``sas_<name>`` for C views; ``sas_<name>_posed`` when they come with pose sets."""
        if pose_sets is None:
            rc = getattr(self._L, name)(self._ctx, C, pV, pK, *tail)
        else:
            Rt, idx = self._pose_sets(pose_sets, pose_set, C)
            rc = getattr(self._L, name + "_posed")(self._ctx, C, pV, pK, idx.ctypes.data, Rt.shape[0], Rt.ctypes.data, *tail)
        if rc != 0:
            self._check(rc, name)

    def _pose_sets(self, pose_sets, pose_set, C: int):
        """(Rt [S,G,12] float32, index [C] int32) of per-view pose sets, validated."""
        Rt = np.ascontiguousarray(np.asarray(_host(pose_sets), dtype=np.float32))
        if self.n_groups <= 0 or Rt.size % (12 * self.n_groups):
            raise ValueError(f"pose_sets must be [S,{self.n_groups},12] for this scene")
        Rt = Rt.reshape(-1, self.n_groups, 12)
        idx = np.ascontiguousarray(np.asarray(pose_set, dtype=np.int32).reshape(-1))
        if idx.shape[0] != C:
            raise ValueError(f"pose_set must name one pose set per view ({C}), got {idx.shape[0]}")
        return Rt, idx

    @_locked
    def render_batch(self, viewmats: ArrayLike, Ks: ArrayLike, width: int, height: int,
                     background: Sequence[float] = (0.0, 0.0, 0.0), *, want: Iterable[str] = ("rgb",),
                     depth_fill_max: bool = False, block: bool = True, time_tiles: bool = False, mesh_surface: bool = False,
                     out: Optional[Dict[str, torch.Tensor]] = None, pose_sets: Optional[ArrayLike] = None,
                     pose_set: Optional[Sequence[int]] = None) -> Dict[str, torch.Tensor]:
        """Render C same-sized views in one C-ABI call: ``viewmats [C,4,4]``, ``Ks [C,3,3]`` ->
        tensors ``[C,H,W,...]`` (the per-camera loop of the reference, splat_env_wrapper.py:147-158).
        Views are projected two per pass over the scene.  ``block=False`` only enqueues (results valid
        after ``wait()``); ``out`` supplies the ``[C,H,W,...]`` output tensors.  ``pose_sets [S,G,12]`` +
        ``pose_set [C]``: view v is rendered with the group poses ``pose_sets[pose_set[v]]`` (vectorised envs:
        sas_render_batch_posed).  ``mesh_surface``: as in ``render``."""
        keep, pV, pK, pbg, C, W, H = self._views(viewmats, Ks, background, width, height, True)
        res, ptrs = self._outputs(want, self._SHAPES, H, W, out, C)
        flags = _flags(block, depth_fill_max, mesh_surface, time_tiles=time_tiles)
        self._batch_call("sas_render_batch", C, pV, pK, pose_sets, pose_set, W, H, pbg, flags,
                         ptrs["rgb"], ptrs["alpha"], ptrs["depth"], ptrs["rgb8"], self._stream())
        self._in_flight(block, res, keep)
        return res

    def _select_onehot_stores(self) -> None:
        """The one-hot group store for the Gaussians and, when the scene holds meshes, for the triangles (replacing features
        uploaded before): what ``render_group_masks`` and ``render_batch_labels`` composite."""
        if not self._features_onehot:
            self.upload_features(None)
        if self.n_mesh_triangles > 0 and not self._mesh_features_onehot:
            self.upload_mesh_features(None)

    @_locked
    def render_batch_labels(self, viewmats: ArrayLike, Ks: ArrayLike, width: int, height: int,
                            background: Sequence[float] = (0.0, 0.0, 0.0), *, min_alpha: float = 0.5,
                            want: Iterable[str] = ("labels",), depth_fill_max: bool = False, mesh_surface: Optional[bool] = None,
                            pose_sets: Optional[ArrayLike] = None, pose_set: Optional[Sequence[int]] = None,
                            out: Optional[Dict[str, torch.Tensor]] = None, timing: bool = False) -> Dict[str, torch.Tensor]:
        """Label frames of C same-sized views in one C-ABI call (sas_render_batch_labels[_posed]): ``labels [C,H,W]`` uint8, per
        pixel the pose group it shows -- ``group_labels`` of what ``render_group_masks`` composites for that view, made on the
        device without the ``[H,W,G]`` weights ever being written -- plus any of ``rgb`` / ``alpha`` / ``depth`` / ``rgb8``
        ``[C,H,W,...]`` listed in ``want`` (bit-identical to ``render_batch`` with the same flags).  ``pose_sets`` +
        ``pose_set``: as in ``render_batch``; the context's poses stay as they are.  ``mesh_surface=None``: on when the scene
        holds meshes (``render_group_masks``' rule: a mesh counts as opaque).  Selects the one-hot stores as
        ``render_group_masks`` does.  Blocking.  ``timing``: per-stage events (``stage_time_means``; timed frames run alone)."""
        self._select_onehot_stores()
        keep, pV, pK, pbg, C, W, H = self._views(viewmats, Ks, background, width, height, True)
        res, ptrs = self._outputs(dict.fromkeys(tuple(want) + ("labels",)), self._LABEL_SHAPES, H, W, out, C)
        surface = self.n_mesh_triangles > 0 if mesh_surface is None else bool(mesh_surface)
        flags = _flags(True, depth_fill_max, surface, timing=timing)
        self._batch_call("sas_render_batch_labels", C, pV, pK, pose_sets, pose_set, W, H, pbg, float(min_alpha), flags,
                         ptrs["rgb"], ptrs["alpha"], ptrs["depth"], ptrs["rgb8"], ptrs["labels"], self._stream())
        self._in_flight(True)
        return res

    def _is_mine(self, t, dtype: torch.dtype, shape: Tuple[int, ...], same_count: bool = False) -> bool:
        """Is ``t`` a contiguous tensor of ``dtype`` and ``shape`` (``same_count``: of as many elements) on this context's device?"""
        return isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and t.device == self.device and \
            (t.numel() == int(np.prod(shape)) if same_count else tuple(t.shape) == tuple(shape))

    def _lift_buffer(self, t: Optional[torch.Tensor], shape: Tuple[int, ...], name: str) -> torch.Tensor:
        """A sum buffer of ``lift_labels``: the caller's (accumulated into), validated, or a zeroed one."""
        if t is None:
            return torch.zeros(shape, dtype=torch.int64, device=self.device)
        if not self._is_mine(t, torch.int64, shape):
            raise ValueError(f"{name} must be a contiguous int64 tensor {shape} on {self.device}")
        return t

    @_locked
    def lift_labels(self, viewmats: ArrayLike, Ks: ArrayLike, width: int, height: int, labels: ArrayLike, n_labels: int, *,
                    votes: Union[torch.Tensor, None, bool] = None, seen: Union[torch.Tensor, None, bool] = None,
                    fast_exp: bool = False, timing: bool = False) -> Dict[str, torch.Tensor]:
        """Lift label images onto the Gaussians (sas_lift_labels), the transpose of a label frame: ``labels [C,H,W]`` uint8 (a
        NumPy array or a tensor; copied to the device as uint8) for the views ``viewmats [C,4,4]``, ``Ks [C,3,3]``.  Every
        Gaussian collects, from every pixel it is composited into, ``q = floor(weight * LIFT_ONE)`` of its compositing weight:
        ``seen [N]`` takes all of them, ``votes [N,n_labels]`` those of pixels labelled below ``n_labels`` (255: unlabelled), in
        the caller's Gaussian order, as int64 device tensors.  ``votes`` / ``seen``: a tensor is ACCUMULATED into (zero it
        once, lift many batches), ``None`` allocates a zeroed one, ``False`` leaves that output out (not both).  Integer sums:
        the result does not depend on the order or the batching of the views.  The context's current group poses apply; a
        scene with meshes is refused (``clear_meshes`` first).  Blocking."""
        keep, pV, pK, _, C, W, H = self._views(viewmats, Ks, (0.0, 0.0, 0.0), width, height, True)
        G = int(n_labels)
        if isinstance(labels, torch.Tensor):
            lab = labels.detach().to(device=self.device, dtype=torch.uint8).contiguous()
        else:
            lab = torch.from_numpy(np.ascontiguousarray(np.asarray(labels, dtype=np.uint8))).to(self.device)
        if lab.numel() != C * H * W:
            raise ValueError(f"labels must be [{C},{H},{W}], got {tuple(lab.shape)}")
        if votes is False and seen is False:
            raise ValueError("lift_labels: votes and seen are both left out")
        res: Dict[str, torch.Tensor] = {}
        if votes is not False:
            res["votes"] = self._lift_buffer(votes, (self.n, max(G, 0)), "votes")
        if seen is not False:
            res["seen"] = self._lift_buffer(seen, (self.n,), "seen")
        stream = self._stream()   # (the frames run behind what this stream holds: the label copy, the zeroing)
        rc = self._L.sas_lift_labels(self._ctx, C, pV, pK, W, H, lab.data_ptr(), G, _flags(True, fast_exp=fast_exp, timing=timing),
                                     res["votes"].data_ptr() if "votes" in res else None,
                                     res["seen"].data_ptr() if "seen" in res else None, stream)
        if rc != 0:
            self._check(rc, "sas_lift_labels")
        self._in_flight(True)
        return res

    @_locked
    def lift_features(self, viewmats: ArrayLike, Ks: ArrayLike, width: int, height: int, images: ArrayLike, *,
                      feature_scale: Optional[float] = None, mask: Optional[ArrayLike] = None,
                      sums: Union[torch.Tensor, None, bool] = None, weight: Union[torch.Tensor, None, bool] = None,
                      fast_exp: bool = False, timing: bool = False) -> Dict[str, Union[torch.Tensor, float]]:
        """Lift feature images onto the Gaussians (sas_lift_features), ``lift_labels`` with real-valued channels: ``images
        [C,H,W,D]`` float32 (a NumPy array or a tensor; ``D`` up to 256) for the views ``viewmats [C,4,4]``, ``Ks [C,3,3]``.
        Every Gaussian collects, from every pixel it is composited into, ``q = floor(weight * LIFT_FEATURE_ONE)`` of its
        compositing weight into ``weight [N]`` and ``q * fq`` into ``sums [N,D]`` (int64 device tensors, the caller's Gaussian
        order), ``fq = rint(clip(f * feature_scale, -32767, 32767))`` the pixel's quantised channels (NaN counts as 0): the
        weighted mean feature is ``sums / (weight * feature_scale)`` (``semantics.features_from_sums``).  ``mask [C,H,W]``: pixels
        where it is 0 add nothing.  ``sums`` / ``weight``: a tensor is ACCUMULATED into, ``None`` allocates a zeroed one,
        ``False`` leaves that output out (not both).  ``feature_scale=None`` picks ``32767 / max|finite f|`` of THIS call's
        images (1 if they are all zero); it is returned as ``"feature_scale"``.  Accumulating over several calls requires
        passing one scale explicitly to all of them: sums made with different scales do not add.  Integer sums: the result
        does not depend on the order or the batching of the views.  No sum can have overflowed while ``weight < 2**48``
        (``features_from_sums`` checks it).  The context's current group poses apply; a scene with meshes is refused.
        Blocking."""
        keep, pV, pK, _, C, W, H = self._views(viewmats, Ks, (0.0, 0.0, 0.0), width, height, True)
        if isinstance(images, torch.Tensor):
            img = images.detach().to(device=self.device, dtype=torch.float32).contiguous()
        else:
            img = torch.from_numpy(np.ascontiguousarray(np.asarray(images, dtype=np.float32))).to(self.device)
        if img.dim() == 3:   # one channel
            img = img[..., None]
        if img.dim() != 4 or tuple(img.shape[:3]) != (C, H, W) or img.shape[3] < 1:
            raise ValueError(f"images must be [{C},{H},{W},D], got {tuple(img.shape)}")
        D = int(img.shape[3])
        m = None
        if mask is not None:
            if isinstance(mask, torch.Tensor):
                m = (mask.detach().to(self.device) != 0).to(torch.uint8).contiguous()
            else:
                m = torch.from_numpy(np.ascontiguousarray((np.asarray(mask) != 0).astype(np.uint8))).to(self.device)
            if m.numel() != C * H * W:
                raise ValueError(f"mask must be [{C},{H},{W}], got {tuple(m.shape)}")
        if feature_scale is None:
            finite = torch.where(torch.isfinite(img), img.abs(), torch.zeros_like(img))
            top = float(finite.max())
            feature_scale = 32767.0 / top if top > 0.0 else 1.0
        scale = float(np.float32(feature_scale))
        if sums is False and weight is False:
            raise ValueError("lift_features: sums and weight are both left out")
        res: Dict[str, Union[torch.Tensor, float]] = {}
        if sums is not False:
            res["sums"] = self._lift_buffer(sums, (self.n, D), "sums")
        if weight is not False:
            res["weight"] = self._lift_buffer(weight, (self.n,), "weight")
        res["feature_scale"] = scale
        stream = self._stream()   # (the frames run behind what this stream holds: the image copy, the zeroing)
        rc = self._L.sas_lift_features(self._ctx, C, pV, pK, W, H, img.data_ptr(), D, scale, m.data_ptr() if m is not None else None,
                                       _flags(True, fast_exp=fast_exp, timing=timing),
                                       res["sums"].data_ptr() if "sums" in res else None,
                                       res["weight"].data_ptr() if "weight" in res else None, stream)
        if rc != 0:
            self._check(rc, "sas_lift_features")
        self._in_flight(True)
        return res

    def _grad_image(self, g, shape: Tuple[int, ...], name: str) -> Optional[torch.Tensor]:
        """A pixel-gradient image of ``render_backward`` on the device, float32, or None."""
        if g is None:
            return None
        t = g.detach() if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(g, dtype=np.float32)))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if t.numel() != int(np.prod(shape)):
            raise ValueError(f"{name} must be {list(shape)}, got {tuple(t.shape)}")
        return t

    @_locked
    def render_backward(self, viewmat: ArrayLike, K: ArrayLike, width: int, height: int, g_rgb=None, g_alpha=None, g_depth=None, *,
                        screen_space: bool = False, out: Optional[Dict[str, torch.Tensor]] = None,
                        want: Optional[Iterable[str]] = None, fast_exp: bool = False,
                        pose_groups: Optional[Sequence[int]] = None) -> Dict[str, torch.Tensor]:
        """The backward pass of one view (sas_render_backward; DESIGN.md 3, "Backward pass").  ``g_rgb [H,W,3]``, ``g_alpha [H,W]``,
        ``g_depth [H,W]`` (tensors or arrays, each may be None, not all) are the gradients of a loss with respect to the frame's RAW
        accumulators: ``sum c alpha T`` (rgb before background and clamp), ``1 - T_final`` and ``sum z alpha T`` (depth before the
        division by alpha); ``autograd.render_differentiable`` does that pre-chain.  Returns float32 device tensors in the caller's
        Gaussian order, with respect to the arrays last uploaded: ``means [N,3]``, ``opacities [N]``, ``colors [N,K,3]`` (the SH
        coefficients; ``[N,1,3]`` plain colours), ``quats [N,4]`` and ``scales [N,3]`` or ``covariances [N,6]`` as the scene was
        uploaded, and ``viewmat [3,4]`` (rows ``[R | t]``, twelve independent entries).  ``screen_space=True`` (sas_render_backward_screen)
        stops in front of the projection: ``means2d [N,2]``, ``conics [N,3]``, ``opacities [N]``, ``colors [N,3]``, ``depths [N]``.
        ``out``: a dict of such tensors to ACCUMULATE into (several views sum); missing keys are allocated zeroed.  ``want``: only
        these keys are computed and returned (the others are NULL to the C call, whose kernels then neither read nor write them):
        a pose optimiser asks for ``("viewmat",)`` alone.
        ``pose_groups``: up to 32 distinct group ids (sas_render_backward_poses); the result gains ``group_poses [n_sel,3,4]``, the
        gradient with respect to the rows ``[R | t]`` of those groups' current poses (twelve independent entries each, as ``viewmat``), in
        the order of ``pose_groups``; ``want`` may name it only then, and ``("group_poses",)`` alone computes nothing else.  More groups:
        call again with the next 32.
        Decisions (culls, clamps, the compositing thresholds) are constants; K, meshes and joint angles are not differentiated (a
        scene with meshes is refused).  The sums over pixels are float atomics: last bits vary from run to run.  Blocking."""
        V, pV = self._host_arg(viewmat, 16)
        Kc, pK = self._host_arg(K, 9)
        W, H = int(width), int(height)
        gr = self._grad_image(g_rgb, (H, W, 3), "g_rgb")
        ga = self._grad_image(g_alpha, (H, W), "g_alpha")
        gd = self._grad_image(g_depth, (H, W), "g_depth")
        if gr is None and ga is None and gd is None:
            raise ValueError("render_backward: g_rgb, g_alpha and g_depth are all None")
        n = self.n
        if screen_space:
            shapes = dict(means2d=(n, 2), conics=(n, 3), opacities=(n,), colors=(n, 3), depths=(n,))
        else:
            scene = self._scene_shapes()
            shapes = {k: scene.pop(k) for k in ("means", "opacities", "colors")}
            shapes.update(viewmat=(3, 4), **scene)   # (the keys keep the order they always had: it shows in results and messages)
        sel = None
        if pose_groups is not None:
            if screen_space:
                raise ValueError("render_backward: pose_groups needs the projection's backward: not with screen_space=True")
            ids = [int(g) for g in pose_groups]
            if not ids or any(g < 0 or g > 255 for g in ids):
                raise ValueError(f"render_backward: pose_groups must name group ids in 0..255, got {tuple(pose_groups)}")
            sel = np.ascontiguousarray(ids, dtype=np.uint8)
            shapes["group_poses"] = (len(ids), 3, 4)
        if want is not None:
            want = tuple(want)
            unknown = [k for k in want if k not in shapes]
            if unknown or not want:
                raise ValueError(f"render_backward: want must name some of {tuple(shapes)}, got {want}")
            shapes = {k: v for k, v in shapes.items() if k in want}
        res: Dict[str, torch.Tensor] = {}
        for name, shape in shapes.items():
            t = out.get(name) if out else None
            if t is None:
                t = torch.zeros(shape, dtype=torch.float32, device=self.device)
            elif not self._is_mine(t, torch.float32, shape):
                raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor {shape} on {self.device}")
            res[name] = t
        flags, stream = _flags(True, fast_exp=fast_exp), self._stream()
        if screen_space:
            rc = self._L.sas_render_backward_screen(self._ctx, pV, pK, W, H, flags, _addr(gr), _addr(ga), _addr(gd), _addr(res.get("means2d")),
                                                    _addr(res.get("conics")), _addr(res.get("opacities")), _addr(res.get("colors")), _addr(res.get("depths")), stream)
        elif sel is not None:
            with_poses = "group_poses" in res   # (left out through ``want``: the plain call)
            rc = self._L.sas_render_backward_poses(self._ctx, pV, pK, W, H, flags, _addr(gr), _addr(ga), _addr(gd), _addr(res.get("means")),
                                                   _addr(res.get("opacities")), _addr(res.get("colors")), _addr(res.get("quats")), _addr(res.get("scales")),
                                                   _addr(res.get("covariances")), _addr(res.get("viewmat")), len(sel) if with_poses else 0,
                                                   sel.ctypes.data if with_poses else None, _addr(res.get("group_poses")), stream)
        else:
            rc = self._L.sas_render_backward(self._ctx, pV, pK, W, H, flags, _addr(gr), _addr(ga), _addr(gd), _addr(res.get("means")), _addr(res.get("opacities")),
                                             _addr(res.get("colors")), _addr(res.get("quats")), _addr(res.get("scales")), _addr(res.get("covariances")),
                                             _addr(res.get("viewmat")), stream)
        if rc != 0:
            self._check(rc, "sas_render_backward_screen" if screen_space else "sas_render_backward_poses" if sel is not None else "sas_render_backward")
        self._in_flight(True)
        return res

    # -- fitting ------------------------------------------------------------------------------
    _ADAM_LRS = ("means", "opacities", "sh_dc", "sh_rest", "quats", "scales")

    def _scene_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """The arrays of the scene last uploaded, by the keys ``render_backward`` and ``read_scene`` use."""
        n = self.n
        kk = (self.sh_degree + 1) ** 2 if self.sh_degree >= 0 else 1
        shapes = dict(means=(n, 3), opacities=(n,), colors=(n, kk, 3))
        shapes.update(dict(quats=(n, 4), scales=(n, 3)) if self.covariance_form == "quats" else dict(covariances=(n, 6)))
        return shapes

    @_locked
    def adam_step(self, grads: Dict[str, torch.Tensor], lrs: Dict[str, float], step: int, betas: Tuple[float, float] = (0.9, 0.999),
                  eps: float = 1e-15, visible_only: bool = False, rest: bool = False) -> None:
        """One fused Adam step on the RESIDENT scene (sas_scene_adam_step; DESIGN.md 3, "Optimiser step"): the next frame shows the
        stepped scene, with no upload.  ``grads``: what ``render_backward`` returns or accumulates into through ``out=`` -- float32
        device tensors under ``means``, ``opacities``, ``colors``, ``quats``, ``scales``, with respect to the activated arrays; other
        keys (``viewmat``) are ignored.  ``lrs``: learning rates under ``means``, ``opacities``, ``sh_dc``, ``sh_rest``, ``quats``,
        ``scales``; a group without a gradient or with rate 0 (or none) is neither read nor written.  The variables are the means,
        log(scales), logit(opacities), the quaternions as uploaded and the SH coefficients; the covariances of a scene uploaded as
        covariances are fixed.  ``step``: 1-based, the caller's count.  ``visible_only``: Gaussians whose gradient is exactly zero
        in every stepped array (culled in every view of the batch) are skipped, moments included.  The moments live in the context
        until ``adam_reset`` or the next ``upload``.  ``n``, ``sh_degree``, groups, group poses, features and meshes stay; the last
        frame's ``read_projection`` / ``read_tile_lists`` do not.  The call only enqueues, on the current stream.
        ``rest=True`` (sas_scene_adam_step_rest): the step on the REST scene of a bound skin -- ``grads`` are then gradients with
        respect to the rest arrays: ``deform_backward_rest``'s ``means`` and ``quats``, and ``render_backward``'s ``opacities``,
        ``colors`` and ``scales`` as they are (a deformation does not touch them).  The same kernel on the same optimiser state; the
        last ``deform`` is applied again to the stepped rest scene, so the next frame and ``read_scene`` show it in its current bend,
        and ``clear_skin`` returns the stepped rest scene.  ``SasError`` without a skin; ``rest=False`` under a skin raises as ever."""
        unknown = [k for k in lrs if k not in self._ADAM_LRS]
        if unknown:
            raise ValueError(f"adam_step: unknown learning rates {unknown}; expected some of {self._ADAM_LRS}")
        shapes = self._scene_shapes()
        ptrs = {}
        for k in ("means", "opacities", "colors", "quats", "scales"):
            t = grads.get(k)
            if t is None:
                ptrs[k] = None
                continue
            if k not in shapes:
                raise ValueError(f"adam_step: the scene was uploaded as covariances, which are not variables: drop grads[{k!r}]")
            if not self._is_mine(t, torch.float32, shapes[k], same_count=True):
                raise ValueError(f"grads[{k!r}] must be a contiguous float32 tensor {shapes[k]} on {self.device}")
            ptrs[k] = t.data_ptr()
        cfg = _capi.AdamConfig(*[float(lrs.get(k, 0.0)) for k in self._ADAM_LRS], float(betas[0]), float(betas[1]), float(eps), int(step),
                               _capi.SAS_ADAM_VISIBLE_ONLY if visible_only else 0)
        entry = "sas_scene_adam_step_rest" if rest else "sas_scene_adam_step"
        rc = getattr(self._L, entry)(self._ctx, ctypes.byref(cfg), ptrs["means"], ptrs["opacities"], ptrs["colors"], ptrs["quats"],
                                     ptrs["scales"], self._stream())
        if rc != 0:
            self._check(rc, entry)
        self._in_flight(True)

    @_locked
    def adam_reset(self) -> None:
        """Drop the optimiser state (sas_scene_adam_reset): the next ``adam_step`` starts from zero moments, with ``step=1``."""
        self._check(self._L.sas_scene_adam_reset(self._ctx), "sas_scene_adam_reset")

    # -- density control ------------------------------------------------------------------------
    _DENSITY_STATS = dict(grad_sum=torch.float32, count=torch.int32, max_radius=torch.float32)
    _DENSIFY_CONFIG = dict(grow_grad2d=2e-4, grow_scale3d=0.01, prune_opacity=0.005, prune_scale3d=0.1, scene_extent=1.0, split_factor=1.6,
                           max_gaussians=0, seed=0, grow=True, prune_opacity_on=True, prune_scale_on=True)

    def new_density_stats(self) -> Dict[str, torch.Tensor]:
        """Zeroed statistics for ``density_accumulate`` / ``densify``: ``grad_sum``, ``max_radius`` (float32) and ``count`` (int32), each
        ``[N]`` on the device, in the caller's order."""
        return {k: torch.zeros(self.n, dtype=dt, device=self.device) for k, dt in self._DENSITY_STATS.items()}

    def _density_stat(self, stats, k: str) -> torch.Tensor:
        t = stats.get(k)
        if not self._is_mine(t, self._DENSITY_STATS[k], (self.n,)):
            raise ValueError(f"stats[{k!r}] must be a contiguous {self._DENSITY_STATS[k]} tensor ({self.n},) on {self.device}: new_density_stats() makes them")
        return t

    @_locked
    def density_accumulate(self, width: int, height: int, stats: Dict[str, torch.Tensor], d_means2d: Optional[torch.Tensor] = None) -> None:
        """Add the last backward frame to the density statistics (sas_density_accumulate; DESIGN.md 3, "Density control"): for every
        Gaussian that frame saw, ``grad_sum += |(0.5 W du, 0.5 H dv)|``, ``count += 1``, ``max_radius = max(max_radius, radius)``.
        ``d_means2d [N,2]``: what ``render_backward(screen_space=True)`` returned for that frame; None: the sums the last
        ``render_backward`` left in the context.  ``stats`` may leave ``max_radius`` out.  Only enqueues, on the current stream."""
        gs, cn = self._density_stat(stats, "grad_sum"), self._density_stat(stats, "count")
        mr = self._density_stat(stats, "max_radius") if stats.get("max_radius") is not None else None
        pm = None
        if d_means2d is not None:
            if not self._is_mine(d_means2d, torch.float32, (self.n, 2)):
                raise ValueError(f"d_means2d must be a contiguous float32 tensor ({self.n}, 2) on {self.device}")
            pm = d_means2d.data_ptr()
        rc = self._L.sas_density_accumulate(self._ctx, int(width), int(height), pm, gs.data_ptr(), cn.data_ptr(),
                                            mr.data_ptr() if mr is not None else None, self._stream())
        if rc != 0:
            self._check(rc, "sas_density_accumulate")

    @_locked
    def densify(self, stats: Dict[str, torch.Tensor], **config) -> Dict[str, object]:
        """Densify and prune the RESIDENT scene by the statistics (sas_scene_densify; DESIGN.md 3, "Density control").  ``config``:
        ``grow_grad2d`` (2e-4), ``grow_scale3d`` (0.01), ``prune_opacity`` (0.005), ``prune_scale3d`` (0.1), ``scene_extent`` (1),
        ``split_factor`` (1.6), ``max_gaussians`` (0: no cap), ``seed`` (0) and the switches ``grow``, ``prune_opacity_on``,
        ``prune_scale_on`` (all on; all off renews the storage order alone).  Returns ``n`` (the new count, also ``self.n``), ``parents``
        (int32 ``[n]`` device: each new Gaussian's old index), ``cloned``, ``split``, ``pruned``.  The optimiser state follows the
        survivors; features are dropped (``upload_features(f[parents])``), ``stats`` has the old length (``new_density_stats()``).
        Blocking."""
        unknown = [k for k in config if k not in self._DENSIFY_CONFIG]
        if unknown:
            raise ValueError(f"densify: unknown settings {unknown}; expected some of {tuple(self._DENSIFY_CONFIG)}")
        cf = dict(self._DENSIFY_CONFIG, **config)
        gs, cn = self._density_stat(stats, "grad_sum"), self._density_stat(stats, "count")
        flags = (_capi.SAS_DENSIFY_GROW if cf["grow"] else 0) | (_capi.SAS_DENSIFY_PRUNE_OPACITY if cf["prune_opacity_on"] else 0) | \
                (_capi.SAS_DENSIFY_PRUNE_SCALE if cf["prune_scale_on"] else 0)
        cfg = _capi.DensifyConfig(float(cf["grow_grad2d"]), float(cf["grow_scale3d"]), float(cf["prune_opacity"]), float(cf["prune_scale3d"]),
                                  float(cf["scene_extent"]), float(cf["split_factor"]), int(cf["max_gaussians"]), int(cf["seed"]) & 0xffffffff, flags)
        parents = torch.empty(max(2 * self.n, 1), dtype=torch.int32, device=self.device)
        counts = (ctypes.c_int64 * 4)()
        rc = self._L.sas_scene_densify(self._ctx, ctypes.byref(cfg), gs.data_ptr(), cn.data_ptr(), parents.data_ptr(), counts, self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_densify")
        self._in_flight(True)
        self.n = int(counts[0])
        self._forget("features")
        self._regroup(parents[:self.n])
        return dict(n=self.n, parents=parents[:self.n], cloned=int(counts[1]), split=int(counts[2]), pruned=int(counts[3]))

    def _regroup(self, parents: torch.Tensor) -> None:
        """The splat-group ids this object remembers (``bind_skin(group=...)`` selects by them) follow a new set of Gaussians: each takes
        its parent's, as the library's do."""
        if self._group_ids is not None:
            self._group_ids = torch.as_tensor(self._group_ids).to(self.device).reshape(-1)[parents.long()]

    @_locked
    def reset_opacity(self, max_opacity: float = 0.01) -> None:
        """Every resident opacity above ``max_opacity`` becomes ``max_opacity`` (sas_scene_reset_opacity), its optimiser state is started
        anew.  Only enqueues, on the current stream."""
        rc = self._L.sas_scene_reset_opacity(self._ctx, float(max_opacity), self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_reset_opacity")
        self._in_flight(True)

    # -- MCMC density control -------------------------------------------------------------------
    _MCMC_CONFIG = dict(min_opacity=0.005, cap_max=1_000_000, grow_factor=1.05, seed=0)

    @_locked
    def mcmc_noise(self, scale: float, step: int, seed: int = 0) -> None:
        """Noise on the RESIDENT means (sas_scene_mcmc_noise; DESIGN.md 3, "MCMC density control"): every mean moves by
        ``C (xi g scale)`` -- ``C`` the Gaussian's own covariance, ``g = sigmoid(-100 (o - 0.005))`` the gate that leaves opaque
        Gaussians where they are, ``xi`` three standard normals keyed by ``(seed, step, the Gaussian's index in the caller's order,
        axis)``: the same key gives the same bits whatever the storage order.  ``scale``: gsplat's ``noise_lr`` times the means' current
        learning rate; 0 changes nothing.  ``step``: 1-based.  The optimiser state is not touched; the last frame's ``read_projection`` /
        ``read_tile_lists`` are gone.  Works on scenes uploaded as covariances too.  Only enqueues, on the current stream."""
        rc = self._L.sas_scene_mcmc_noise(self._ctx, float(scale), int(step), int(seed) & 0xffffffff, self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_mcmc_noise")
        self._in_flight(True)

    @_locked
    def mcmc_refine(self, **config) -> Dict[str, object]:
        """Relocate the dead Gaussians of the RESIDENT scene onto alive ones and grow the set towards a cap (sas_scene_mcmc_refine;
        DESIGN.md 3, "MCMC density control").  ``config``: ``min_opacity`` (0.005: at or below it a Gaussian is dead), ``cap_max``
        (1 000 000), ``grow_factor`` (1.05) and ``seed`` (0).  ``n_dead + n_grow`` alive Gaussians are drawn in proportion to their
        opacity; a drawn one and its children share its opacity and shrink (gsplat's ``compute_relocation``).  Returns ``n`` (the new
        count, also ``self.n``; never above ``max(cap_max, the old n)``), ``relocated``, ``added`` and ``parents`` (int32 ``[n]`` device:
        each new Gaussian's old index).  Gaussians that were neither drawn nor born keep their optimiser state, the others start anew;
        features are dropped (``upload_features(f[parents])``).  Refused for a scene uploaded as covariances.  Blocking."""
        unknown = [k for k in config if k not in self._MCMC_CONFIG]
        if unknown:
            raise ValueError(f"mcmc_refine: unknown settings {unknown}; expected some of {tuple(self._MCMC_CONFIG)}")
        cf = dict(self._MCMC_CONFIG, **config)
        cfg = _capi.McmcConfig(int(cf["cap_max"]), float(cf["grow_factor"]), float(cf["min_opacity"]), int(cf["seed"]) & 0xffffffff)
        room = self.n
        if math.isfinite(cfg.grow_factor) and cfg.grow_factor >= 1.0:   # (anything else is refused below)
            room = max(room, int(min(float(cfg.cap_max), cfg.grow_factor * self.n)))   # (clamped as a float, then floored: the product may be inf)
        parents = torch.empty(max(room, 1), dtype=torch.int32, device=self.device)
        counts = (ctypes.c_int64 * 3)()
        rc = self._L.sas_scene_mcmc_refine(self._ctx, ctypes.byref(cfg), parents.data_ptr(), counts, self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_mcmc_refine")
        self._in_flight(True)
        if int(counts[1]) or int(counts[2]):
            self._forget("features")
        self.n = int(counts[0])
        self._regroup(parents[:self.n])
        return dict(n=self.n, relocated=int(counts[1]), added=int(counts[2]), parents=parents[:self.n])

    @_locked
    def photometric_loss(self, rgb, target, *, mask=None, alpha=None, background: Sequence[float] = (0.0, 0.0, 0.0),
                         lambda_dssim: float = 0.2, want_grad: bool = True) -> Dict[str, torch.Tensor]:
        """The 3DGS photometric loss ``(1 - lambda) L1 + lambda (1 - SSIM)`` of a frame ``rgb [H,W,3]`` against ``target [H,W,3]`` and
        its gradient, on the device (sas_photometric_loss; DESIGN.md 3, "Photometric loss").  ``mask [H,W]`` (bool or integer,
        non-zero counts) weights the per-pixel maps; the window statistics see the whole image.  Returns ``terms`` (device float32[4]:
        loss, l1, ssim, mse) and ``loss``, ``l1``, ``ssim``, ``mse`` as 0-d views of it; with ``want_grad`` (a bool, or the names wanted
        of ``g_rgb``, ``g_alpha``) also ``g_rgb [H,W,3]``, the exact derivative of ``loss`` with respect to ``rgb``.  With ``alpha`` (the frame's own, ``render``'s output) the gradient
        is PRECHAINED as ``autograd.prechain`` does with no depth gradient -- ``g_rgb`` is zero where ``rgb >= 1`` and
        ``g_alpha [H,W] = -sum_c g_rgb[c] background[c]`` comes with it: both go straight to ``render_backward``.
        ``lambda_dssim = 0`` is the L1 loss alone and does no SSIM work (``ssim`` is NaN).  Nothing is summed with atomics: the same
        inputs give the same bits.  Non-finite pixels propagate: the terms become NaN, and the gradients within 10 pixels.  The call
        only enqueues, on the current stream; nothing is read back."""
        shape = tuple(rgb.shape) if hasattr(rgb, "shape") else np.asarray(rgb).shape
        if len(shape) != 3 or shape[2] != 3 or min(shape) <= 0:
            raise ValueError(f"rgb must be [H,W,3], got {shape}")
        H, W = int(shape[0]), int(shape[1])
        lam = float(lambda_dssim)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"lambda_dssim {lambda_dssim} outside [0, 1]")
        x = self._grad_image(rgb, (H, W, 3), "rgb")
        y = self._grad_image(target, (H, W, 3), "target")
        a = self._grad_image(alpha, (H, W), "alpha")
        m = None
        if mask is not None:
            m = mask.detach() if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
            if m.numel() != H * W:
                raise ValueError(f"mask must be {[H, W]}, got {tuple(m.shape)}")
            m = m.to(self.device).contiguous()
            m = m.view(torch.uint8) if m.dtype == torch.bool else m if m.dtype == torch.uint8 else (m != 0).view(torch.uint8)
        bg, pbg = self._host_arg(background, 3)
        terms = torch.empty(4, dtype=torch.float32, device=self.device)
        res = dict(terms=terms, loss=terms[0], l1=terms[1], ssim=terms[2], mse=terms[3])
        grads = (("g_rgb", "g_alpha") if a is not None else ("g_rgb",)) if want_grad is True else tuple(want_grad or ())
        if [k for k in grads if k not in ("g_rgb", "g_alpha")]:
            raise ValueError(f"want_grad must be a bool or name some of ('g_rgb', 'g_alpha'), got {want_grad}")
        if "g_alpha" in grads and a is None:
            raise ValueError("g_alpha belongs to the prechained form: pass the frame's alpha")
        for k in grads:
            res[k] = torch.empty((H, W, 3) if k == "g_rgb" else (H, W), dtype=torch.float32, device=self.device)
        rc = self._L.sas_photometric_loss(self._ctx, W, H, x.data_ptr(), y.data_ptr(), _addr(m), _addr(a), pbg, lam, terms.data_ptr(),
                                          _addr(res.get("g_rgb")), _addr(res.get("g_alpha")), self._stream())
        if rc != 0:
            self._check(rc, "sas_photometric_loss")
        return res

    @_locked
    def read_scene(self) -> Dict[str, torch.Tensor]:
        """The resident scene as float32 device tensors in the caller's order and ``upload``'s shapes (sas_scene_read): ``means``,
        ``opacities``, ``colors [N,K,3]`` and ``quats`` + ``scales`` or ``covariances [N,6]``.  Straight after ``upload``: the uploaded
        bits.  After ``adam_step``s: the fitted scene -- save it, or ``upload(**r.read_scene(), sh_degree=r.sh_degree, ...)`` to renew
        the storage order once the means have moved far."""
        res = {k: torch.empty(s, dtype=torch.float32, device=self.device) for k, s in self._scene_shapes().items()}
        p = lambda k: res[k].data_ptr() if k in res and res[k].numel() else None
        torch.cuda.synchronize(self.device)   # (the allocator may hand out memory that work in flight still uses)
        self._check(self._L.sas_scene_read(self._ctx, p("means"), p("quats"), p("scales"), p("covariances"), p("opacities"), p("colors")),
                    "sas_scene_read")
        return res

    @_locked
    def storage_order(self, means: ArrayLike, group_id: Optional[ArrayLike] = None) -> torch.Tensor:
        """The storage order ``upload`` would give these ``means [N,3]`` and ``group_id [N]`` (uint8; None: no groups), computed on the
        device (sas_storage_order; DESIGN.md 3, "Storage order"): int32 ``[N]`` on the device, slot -> the caller's index, ordered by
        (group, Hilbert index of the mean, index).  Device tensors are read where they are.  Needs no scene.  Only enqueues, on the
        current stream (a call at a larger N than any before first grows the context's scratch, which waits for the device)."""
        m = (means.detach() if isinstance(means, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(means, dtype=np.float32))))
        m = m.to(device=self.device, dtype=torch.float32).contiguous()
        if m.dim() != 2 or m.shape[1] != 3:
            raise ValueError(f"means must be [N,3], got {list(m.shape)}")
        n = int(m.shape[0])
        g = None
        if group_id is not None:
            g = group_id.detach() if isinstance(group_id, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(group_id, dtype=np.uint8)))
            g = g.to(device=self.device, dtype=torch.uint8).contiguous()
            if g.numel() != n:
                raise ValueError(f"group_id must be [{n}], got {list(g.shape)}")
        perm = torch.empty(n, dtype=torch.int32, device=self.device)
        rc = self._L.sas_storage_order(self._ctx, n, _addr(m), _addr(g), _addr(perm), self._stream())
        if rc != 0:
            self._check(rc, "sas_storage_order")
        return perm   # (m and g were made on this stream or are the caller's: the allocator hands their memory on behind the kernels)

    @_locked
    def knn_points(self, points: ArrayLike, k: int = 3, indices: bool = True) -> Dict[str, torch.Tensor]:
        """For every point of ``points [N,3]`` its ``k`` (1..8) nearest OTHER points of the same cloud, exactly (sas_knn_points; DESIGN.md
        3, "Scene from points"): ``dist2`` float32 ``[N,k]`` ascending and, with ``indices``, ``index`` int32 ``[N,k]``, device tensors.
        ``d2 = (dx*dx + dy*dy) + dz*dz`` in float32; equal distances go to the lower index; the point itself is left out by index, so a
        duplicate is a neighbour at 0; a point with a non-finite coordinate neither is a neighbour nor has one; a missing neighbour reads
        ``+inf`` / ``-1``.  Device tensors are read where they are.  Needs no scene.  Only enqueues, on the current stream (a call at a
        larger N than any before first grows the context's scratch, which waits for the device)."""
        p = (points.detach() if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float32))))
        p = p.to(device=self.device, dtype=torch.float32).contiguous()
        if p.dim() != 2 or p.shape[1] != 3:
            raise ValueError(f"points must be [N,3], got {list(p.shape)}")
        n, k = int(p.shape[0]), int(k)
        res = {"dist2": torch.empty((n, max(k, 0)), dtype=torch.float32, device=self.device)}
        if indices:
            res["index"] = torch.empty((n, max(k, 0)), dtype=torch.int32, device=self.device)
        rc = self._L.sas_knn_points(self._ctx, n, _addr(p), k, _addr(res["dist2"]), _addr(res.get("index")), self._stream())
        if rc != 0:
            self._check(rc, "sas_knn_points")
        return res   # (p was made on this stream or is the caller's: the allocator hands its memory on behind the kernels)

    @_locked
    def knn_stats(self) -> Dict[str, object]:
        """What the last ``knn_points`` decided on the device (sas_knn_last_counts; blocking): ``leftover`` points its grid search handed
        to the brute-force kernel, the ``grid``'s cells per axis, ``brute`` (no grid: the whole cloud went through the brute-force
        kernel) and the ``occupied`` cells of the 32^3 and 16^3 occupancy grids the grid was chosen from."""
        out = np.zeros(7, np.int64)
        self._check(self._L.sas_knn_last_counts(self._ctx, out.ctypes.data, 7), "sas_knn_last_counts")
        return {"leftover": int(out[0]), "grid": tuple(int(v) for v in out[1:4]), "brute": bool(out[4]), "occupied": (int(out[5]), int(out[6]))}

    # -- deformable splats ----------------------------------------------------------------------
    def _cloud(self, a: ArrayLike, name: str) -> torch.Tensor:
        """``a [N,3]`` as a contiguous float32 tensor on this context's device (a device tensor that is one already: itself)."""
        t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must be [N,3], got {list(t.shape)}")
        return t

    @_locked
    def knn_nodes(self, points: ArrayLike, nodes: ArrayLike, k: int = 4, max_distance: float = math.inf,
                  indices: bool = True) -> Dict[str, torch.Tensor]:
        """For every point of ``points [N,3]`` its ``k`` (1..8) nearest of ``nodes [M,3]`` (1 <= M <= 65536), exactly (sas_knn_cross;
        DESIGN.md 3, "Deformation"): ``dist2`` float32 ``[N,k]`` ascending and, with ``indices``, ``index`` int32 ``[N,k]``, device
        tensors.  ``knn_points``' contract -- ``d2 = (dx*dx + dy*dy) + dz*dz`` in float32, equal distances to the lower index, a
        non-finite ``d2`` never counts, a missing neighbour reads ``+inf`` / ``-1`` -- but nothing is left out by index, and a node
        farther than ``max_distance`` never counts.  ``M < k`` leaves the last columns missing.  Device tensors are read where they
        are.  Needs no scene.  Only enqueues, on the current stream."""
        p, q = self._cloud(points, "points"), self._cloud(nodes, "nodes")
        n, m, k = int(p.shape[0]), int(q.shape[0]), int(k)
        res = {"dist2": torch.empty((n, max(k, 0)), dtype=torch.float32, device=self.device)}
        if indices:
            res["index"] = torch.empty((n, max(k, 0)), dtype=torch.int32, device=self.device)
        rc = self._L.sas_knn_cross(self._ctx, n, _addr(p), m, _addr(q), k, float(max_distance), _addr(res["dist2"]), _addr(res.get("index")),
                                   self._stream())
        if rc != 0:
            self._check(rc, "sas_knn_cross")
        return res   # (p and q were made on this stream or are the caller's: the allocator hands their memory on behind the kernel)

    @property
    def has_skin(self) -> bool:
        """A skin is bound to the resident scene (``set_skin`` / ``bind_skin``; ``clear_skin`` and ``upload`` end it)."""
        return self._skin_k > 0

    @_locked
    def set_skin(self, indices: ArrayLike, weights: ArrayLike) -> None:
        """Bind the resident scene to control nodes (sas_scene_skin; DESIGN.md 3, "Deformation"): ``indices [N,k]`` (integers; int32
        device tensors are read where they are) and ``weights [N,k]`` (float32), ``1 <= k <= 8``, in ``upload``'s order.  An entry counts
        in ``deform`` when ``0 <= index < m`` and ``weight > 0``; anything else is ignored.  The first bind keeps the scene as it stands
        as the REST pose; a bind over a skin replaces the entries and keeps the rest pose.  While a skin is bound ``adam_step`` (but for ``rest=True``),
        ``densify``, ``mcmc_refine``, ``mcmc_noise`` and ``reset_opacity`` raise.  Only enqueues, on the current stream."""
        def dev(a, dt, name):
            t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
            if t.dim() != 2 or t.shape[0] != self.n or not 1 <= t.shape[1] <= _capi.SAS_SKIN_MAX_K:
                raise ValueError(f"{name} must be [{self.n}, k] with 1 <= k <= {_capi.SAS_SKIN_MAX_K}, got {list(t.shape)}")
            if dt == torch.int32 and (t.dtype.is_floating_point or t.dtype == torch.bool):
                raise ValueError(f"{name} must hold integers, got {t.dtype}")
            return t.to(device=self.device, dtype=dt).contiguous()
        i, w = dev(indices, torch.int32, "indices"), dev(weights, torch.float32, "weights")
        if i.shape != w.shape:
            raise ValueError(f"indices {list(i.shape)} and weights {list(w.shape)} differ in shape")
        rc = self._L.sas_scene_skin(self._ctx, int(i.shape[1]), _addr(i), _addr(w), self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_skin")
        self._skin_k = int(i.shape[1])
        self._deform_m = 0
        self._in_flight(True)

    @_locked
    def read_skin(self) -> Dict[str, torch.Tensor]:
        """The bound skin in ``upload``'s order (sas_scene_skin_read): ``indices`` int32 and ``weights`` float32, ``[N,k]`` device
        tensors, the bits ``set_skin`` was given.  Blocking."""
        if not self.has_skin:
            raise SasError("read_skin: no skin is bound")
        res = {"indices": torch.empty((self.n, self._skin_k), dtype=torch.int32, device=self.device),
               "weights": torch.empty((self.n, self._skin_k), dtype=torch.float32, device=self.device)}
        torch.cuda.synchronize(self.device)   # (the allocator may hand out memory that work in flight still uses)
        if self.n:
            self._check(self._L.sas_scene_skin_read(self._ctx, _addr(res["indices"]), _addr(res["weights"])), "sas_scene_skin_read")
        return res

    @_locked
    def clear_skin(self) -> None:
        """Unbind the skin: the rest pose returns bit for bit (as ``adam_step(rest=True)`` has stepped it, if it has), and the calls a
        skin refuses work again.  Without a skin: nothing.  Only enqueues, on the current stream."""
        rc = self._L.sas_scene_skin(self._ctx, 0, None, None, self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_skin")
        self._skin_k = self._deform_m = 0
        self._in_flight(True)

    @_locked
    def deform(self, node_transforms: ArrayLike) -> None:
        """Move the skinned scene (sas_scene_deform; DESIGN.md 3, "Deformation"): ``node_transforms [m,3,4]``, rows ``[R | t]`` that map
        the REST pose to the current one in the frame of ``upload`` (in front of the group poses).  Means follow by linear blend
        skinning over each Gaussian's live entries, orientations by the blended quaternion; the transforms are expected to be rigid
        (stretch and shear are dropped).  Always rest -> current: two calls do not accumulate.  A float32 device tensor is read where
        it is, unchecked; NumPy arrays and lists are copied and checked (``deform.check_node_transforms``: shape, finite, ``R^T R``
        within 1e-4 of identity).  The next frame shows the deformed scene; ``read_scene`` returns it.  Only enqueues, on the current
        stream."""
        if isinstance(node_transforms, torch.Tensor) and node_transforms.is_cuda:
            t = node_transforms.detach()
            if not (t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device and t.dim() == 3 and tuple(t.shape[1:]) == (3, 4)):
                raise ValueError(f"node_transforms on the device must be a contiguous float32 tensor [m,3,4] on {self.device}, got {t.dtype} {list(t.shape)}")
        else:
            from .deform import check_node_transforms
            t = torch.from_numpy(check_node_transforms(_host(node_transforms))).to(self.device)
        m = int(t.shape[0])
        if not 1 <= m <= _capi.SAS_KNN_CROSS_MAX_NODES:
            raise ValueError(f"node_transforms: m={m} out of [1, {_capi.SAS_KNN_CROSS_MAX_NODES}]")
        rc = self._L.sas_scene_deform(self._ctx, m, _addr(t), self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_deform")
        if self.n:
            self._deform_m = m
        self._in_flight(True)

    def _deform_grads(self, who: str, grads, out=None) -> Dict[str, Optional[torch.Tensor]]:
        """What ``deform_backward`` and ``deform_backward_rest`` check alike: ``grads`` (and ``out``, where given) a dict, a skin and a
        ``deform`` since the bind, no gradient of the other orientation form.  Returns ``grads``' checked tensor, or None, under each of
        ``means``, ``quats`` and ``covariances``: not all are None."""
        if not isinstance(grads, dict):
            raise ValueError(f"{who}: grads must be a dict as render_backward returns it")
        if out is not None and not isinstance(out, dict):
            raise ValueError(f"{who}: out must be a dict of tensors to accumulate into")
        if not self.has_skin:
            raise SasError(f"{who}: no skin is bound")
        if self._deform_m <= 0:
            raise SasError(f"{who}: no deform since the skin was bound")
        shapes = self._scene_shapes()
        other = "covariances" if self.covariance_form == "quats" else "quats"
        if grads.get(other) is not None:
            raise ValueError(f"{who}: the scene was uploaded as {'quats' if other == 'covariances' else 'covariances'}: drop grads[{other!r}]")
        given = {}
        for k in ("means", "quats", "covariances"):
            t = grads.get(k)
            if t is not None and not self._is_mine(t, torch.float32, shapes[k]):
                raise ValueError(f"grads[{k!r}] must be a contiguous float32 tensor {shapes[k]} on {self.device}")
            given[k] = t
        if all(t is None for t in given.values()):
            raise ValueError(f"{who}: grads holds neither means nor the orientation gradient")
        return given

    @_locked
    def deform_backward(self, grads: Dict[str, torch.Tensor]) -> torch.Tensor:
        """The adjoint of the last ``deform`` (sas_scene_deform_backward; DESIGN.md 3, "Deformation"): from the gradients of the DEFORMED
        arrays to the gradient of the node transforms, ``[m,3,4]`` float32 on the device, rows ``[dR | dt]``, the twelve entries of every
        node independent variables as ``viewmat``'s and ``group_poses``' are.  ``grads``: the dict ``render_backward`` returns or
        accumulates through ``out=`` on the skinned scene; ``means`` and ``quats`` (or ``covariances``, as the scene was uploaded) are
        read, contiguous float32 device tensors of the scene's shapes; a missing key is left out (not both: without an orientation
        gradient the rotation path is skipped), other keys are ignored.  The adjoint is linear, so several views need no ``out=`` here:
        accumulate ``render_backward(..., out=acc, want=("means", "quats"))`` over the views and call ``deform_backward(acc)`` once.
        What is differentiated is ``deform`` as evaluated, with the live entries, the quaternion branch of every node, the signs and
        the fallback as constants; the state is the node records ``deform`` left on the device, not the caller's tensor.  A node no live
        entry names gets an exact zero row, zero gradients give exact zeros; otherwise the sums are float atomics and vary in their
        last bits from run to run.  ``SasError`` without a skin or without a ``deform`` since the bind.  Only enqueues, on the current
        stream."""
        ptrs = {k: None if t is None else t.data_ptr() for k, t in self._deform_grads("deform_backward", grads).items()}
        out = torch.empty((self._deform_m, 3, 4), dtype=torch.float32, device=self.device)
        rc = self._L.sas_scene_deform_backward(self._ctx, ptrs["means"], ptrs["quats"], ptrs["covariances"], _addr(out), self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_deform_backward")
        return out

    @_locked
    def deform_backward_rest(self, grads: Dict[str, torch.Tensor], out: Optional[Dict[str, torch.Tensor]] = None,
                             bound_only: bool = False) -> Dict[str, torch.Tensor]:
        """The adjoint of the last ``deform`` to the REST scene (sas_scene_deform_backward_rest; DESIGN.md 3, "Deformation"): from the
        gradients of the DEFORMED arrays, the dict ``render_backward`` returns or accumulates on the skinned scene, to the gradients of
        the Gaussians that are stored.  Returns a dict with ``means`` and ``quats`` (or ``covariances``, as the scene was uploaded) for
        the keys ``grads`` holds, float32 device tensors of the scene's shapes; a missing key is left out (not both), other keys are
        ignored: the ``opacities``, ``colors`` and ``scales`` gradients are untouched by a deformation and are the rest scene's as they
        stand.  ``out``: a dict of such tensors to ACCUMULATE into -- every time step has its own deformation, so the sum over time
        steps is taken here: ``deform(T_t)``, the views' ``render_backward(out=acc_t)``, ``deform_backward_rest(acc_t, out=rest_acc)``
        per step, then one ``adam_step(rest_acc, ..., rest=True)``.  Missing keys are allocated zeroed; a tensor of ``out`` must not be
        one of ``grads``.  A Gaussian without a live entry has its gradient passed through bit for bit; ``bound_only=True``: it adds
        nothing (skins bound with ``group=``: the static rest of the scene is then not stepped).  An all-zero gradient adds exact zeros.
        No atomics: the same inputs give the same bits on every run.  ``SasError`` without a skin or without a ``deform`` since the
        bind.  Only enqueues, on the current stream."""
        shapes = self._scene_shapes()
        ptrs, res = {}, {}
        for k, t in self._deform_grads("deform_backward_rest", grads, out).items():
            ptrs[k] = ptrs["o_" + k] = None
            if t is None:
                continue
            o = out.get(k) if out else None
            if o is None:
                o = torch.zeros(shapes[k], dtype=torch.float32, device=self.device)
            elif not self._is_mine(o, torch.float32, shapes[k]):
                raise ValueError(f"out[{k!r}] must be a contiguous float32 tensor {shapes[k]} on {self.device}")
            res[k] = o
            ptrs[k], ptrs["o_" + k] = t.data_ptr(), o.data_ptr()
        if self.n == 0:
            return res
        rc = self._L.sas_scene_deform_backward_rest(self._ctx, ptrs["means"], ptrs["quats"], ptrs["covariances"], ptrs["o_means"], ptrs["o_quats"],
                                                    ptrs["o_covariances"], _capi.SAS_DEFORM_REST_BOUND_ONLY if bound_only else 0, self._stream())
        if rc != 0:
            self._check(rc, "sas_scene_deform_backward_rest")
        return res

    @_locked
    def bind_skin(self, nodes: ArrayLike, k: int = 4, sigma: Optional[float] = None, max_distance: float = math.inf,
                  group: Optional[int] = None) -> Dict[str, object]:
        """Bind every Gaussian to its ``k`` nearest of ``nodes [M,3]`` (the scene's frame, rest pose) with radial weights, and
        ``set_skin`` the result: the rest means come from ``read_scene()``, the neighbours from ``knn_nodes``, and
        ``w_j = exp(-(d2_j - d2_0) / (2 sigma^2))`` -- the nearest node's weight is exactly 1, so no row underflows to a zero sum.
        Missing neighbours (beyond ``max_distance``, or ``M < k``) and Gaussians outside ``group`` (a splat group id of ``upload``; None:
        all) get index -1 and weight 0: they stay at rest.  ``sigma`` None: the mean distance of a node to its nearest other node
        (``knn_points(nodes, 1)``; 1 for a single node).  A skin bound already is cleared first: the nodes are matched against the rest
        pose.  Returns ``indices``, ``weights`` (device tensors) and ``sigma``.  Blocking."""
        q = self._cloud(nodes, "nodes")
        if sigma is None:
            d2 = self.knn_points(q, 1)["dist2"].cpu().numpy().astype(np.float64).reshape(-1)
            d2 = d2[np.isfinite(d2)]
            sigma = float(np.mean(np.sqrt(d2))) if d2.size else 1.0
        sigma = float(sigma)
        if not (sigma > 0.0 and math.isfinite(sigma)):
            raise ValueError(f"sigma must be positive and finite, got {sigma} (coincident nodes? pass sigma)")
        keep = None
        if group is not None:
            if self._group_ids is None or not 0 <= int(group) < self.n_groups:
                raise ValueError(f"group {group}: the scene has {self.n_groups} splat groups")
            keep = torch.as_tensor(self._group_ids).to(self.device).reshape(-1) == int(group)
        self.clear_skin()   # (a skin bound already: back to the rest pose, which is what the nodes are matched against)
        nn = self.knn_nodes(self.read_scene()["means"], q, k, max_distance)
        d2, idx = nn["dist2"], nn["index"]
        w = torch.exp(-(d2 - d2[:, :1]) / (2.0 * sigma * sigma))
        off = idx < 0
        if keep is not None:
            off = off | ~keep[:, None]
        w = torch.where(off, torch.zeros_like(w), w)
        idx = torch.where(off, torch.full_like(idx, -1), idx)
        self.set_skin(idx, w)
        return {"indices": idx, "weights": w, "sigma": sigma}

    def _node_array(self, t, dtype: torch.dtype, shape: Tuple[int, ...], name: str) -> torch.Tensor:
        """``t`` as it is, if it is a contiguous device tensor of ``dtype`` and ``shape`` on this context's device; ValueError otherwise."""
        if not self._is_mine(t, dtype, shape):
            raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} tensor {list(shape)} on {self.device}")
        return t

    @_locked
    def node_rigidity(self, nodes: torch.Tensor, transforms64: torch.Tensor, neighbours: Optional[torch.Tensor] = None,
                      rev_start: Optional[torch.Tensor] = None, rev_edge: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The rigidity term of a deformation graph and its gradient on the device (sas_nodes_rigidity; DESIGN.md 3, "Deformation"):
        what ``deform.rigidity(nodes, T, table=neighbours)`` evaluates, in float64.  Device tensors, read where they are: ``nodes [M,3]``
        float32, ``transforms64 [M,3,4]`` float64, ``neighbours [M,kn]`` int32 (``0 <= kn <= 8``; an entry outside ``[0, M)`` is ignored;
        None: no edges) and its reverse table as ``deform.reverse_table`` builds it: ``rev_start [M+1]`` int32 and ``rev_edge [M*kn]``
        int32, of which the first ``rev_start[M]`` entries are read.  Returns ``value`` (a float64 device scalar) and ``d_transforms
        [M,3,4]`` float64 (``out``: the tensor to write it to).  No atomics: the same inputs give the same bits.  Needs no
        scene.  Only enqueues, on the current stream."""
        if not isinstance(nodes, torch.Tensor) or nodes.dim() != 2:
            raise ValueError("nodes must be a float32 device tensor [M,3]")
        m = int(nodes.shape[0])
        kn = 0 if neighbours is None else int(neighbours.shape[1]) if isinstance(neighbours, torch.Tensor) and neighbours.dim() == 2 else -1
        if not 1 <= m <= _capi.SAS_KNN_CROSS_MAX_NODES:
            raise ValueError(f"node_rigidity: m={m} out of [1, {_capi.SAS_KNN_CROSS_MAX_NODES}]")
        if not 0 <= kn <= _capi.SAS_NODES_MAX_K:
            raise ValueError(f"node_rigidity: neighbours must be [M,kn] with 0 <= kn <= {_capi.SAS_NODES_MAX_K}")
        g = self._node_array(nodes, torch.float32, (m, 3), "nodes")
        T = self._node_array(transforms64, torch.float64, (m, 3, 4), "transforms64")
        nb = rs = re = None
        if kn > 0:
            nb = self._node_array(neighbours, torch.int32, (m, kn), "neighbours")
            rs = self._node_array(rev_start, torch.int32, (m + 1,), "rev_start")
            re = self._node_array(rev_edge, torch.int32, (m * kn,), "rev_edge")
        d = torch.empty((m, 3, 4), dtype=torch.float64, device=self.device) if out is None else self._node_array(out, torch.float64, (m, 3, 4), "out")
        v = torch.empty(1, dtype=torch.float64, device=self.device)
        rc = self._L.sas_nodes_rigidity(self._ctx, m, _addr(g), _addr(T), kn, _addr(nb), _addr(rs), _addr(re), _addr(d), _addr(v), self._stream())
        if rc != 0:
            self._check(rc, "sas_nodes_rigidity")
        return {"value": v[0], "d_transforms": d}

    @_locked
    def node_twist_step(self, nodes: torch.Tensor, transforms64: torch.Tensor, m1: torch.Tensor, m2: torch.Tensor, transforms32: torch.Tensor,
                        d_transforms: Optional[torch.Tensor] = None, d_transforms64: Optional[torch.Tensor] = None, weight64: float = 1.0, *,
                        lr: Tuple[float, float], c1: float, c2: float, beta1: float = 0.9, beta2: float = 0.999, gain1: float = 0.1,
                        gain2: float = 0.001, eps: float = 1e-12) -> None:
        """One Adam step of every node's se(3) twist about the node's current position, on the device (sas_nodes_twist_step; DESIGN.md
        3, "Deformation"): ``deform._twist_step``'s operations per node, in float64.  Device tensors: ``nodes [M,3]`` float32; the
        state ``transforms64 [M,3,4]``, ``m1``, ``m2 [M,6]`` float64, stepped IN PLACE; ``transforms32 [M,3,4]`` float32, written: the
        stepped transforms rounded once, what ``deform`` takes.  The gradient is ``double(d_transforms) + weight64 * d_transforms64``
        (float32 / float64 ``[M,3,4]``; either may be None, not both).  ``lr``: the (rotation, translation) rates of this step, decay
        included; ``c1``, ``c2``: Adam's bias corrections ``1 - beta ** (it + 1)``; ``gain``: the weight of the new gradient in a
        moment.  Needs no scene.  Only enqueues, on the current stream."""
        if not isinstance(nodes, torch.Tensor) or nodes.dim() != 2:
            raise ValueError("nodes must be a float32 device tensor [M,3]")
        m = int(nodes.shape[0])
        if not 1 <= m <= _capi.SAS_KNN_CROSS_MAX_NODES:
            raise ValueError(f"node_twist_step: m={m} out of [1, {_capi.SAS_KNN_CROSS_MAX_NODES}]")
        g = self._node_array(nodes, torch.float32, (m, 3), "nodes")
        T = self._node_array(transforms64, torch.float64, (m, 3, 4), "transforms64")
        a1, a2 = self._node_array(m1, torch.float64, (m, 6), "m1"), self._node_array(m2, torch.float64, (m, 6), "m2")
        T32 = self._node_array(transforms32, torch.float32, (m, 3, 4), "transforms32")
        d32 = None if d_transforms is None else self._node_array(d_transforms, torch.float32, (m, 3, 4), "d_transforms")
        d64 = None if d_transforms64 is None else self._node_array(d_transforms64, torch.float64, (m, 3, 4), "d_transforms64")
        if d32 is None and d64 is None:
            raise ValueError("node_twist_step: one of d_transforms and d_transforms64 is required")
        cfg = _capi.NodeStepConfig(float(lr[0]), float(lr[1]), float(beta1), float(beta2), float(c1), float(c2), float(eps), float(gain1), float(gain2))
        rc = self._L.sas_nodes_twist_step(self._ctx, m, _addr(g), _addr(d32), _addr(d64), float(weight64), _addr(T), _addr(a1), _addr(a2), _addr(T32),
                                          ctypes.byref(cfg), self._stream())
        if rc != 0:
            self._check(rc, "sas_nodes_twist_step")

    @_locked
    def node_fit_rigid(self, nodes: torch.Tensor, moved: torch.Tensor, table: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       out64: Optional[torch.Tensor] = None, want64: bool = True) -> Dict[str, Optional[torch.Tensor]]:
        """Every node's rigid ``[R | t]``, rest -> moved, from node POSITIONS on the device (sas_nodes_fit_rigid; DESIGN.md 3,
        "Deformation"): what ``deform.transforms_from_positions(nodes, moved, table=table)`` computes, without the host.  Device tensors, read
        where they are: ``nodes [M,3]`` float32, ``moved [M,3]`` or ``[S,M,3]`` float32 (``S`` time steps in one launch), ``table [M,kn]``
        int32 (``0 <= kn <= 8``, ``knn_points``' table; an entry outside ``[0, M)`` is ignored; None: no neighbours, every rotation the
        identity).  A member whose moved position is not finite is left out of its neighbours' fits; a node whose OWN moved position is not
        finite gets ``[I | 0]``.  A collinear neighbourhood (two nodes, a rope) gets the LEAST rotation of all optimal ones.  Returns
        ``transforms64`` (float64) and ``transforms`` (float32, the float64 rounded once: what ``deform`` takes), ``[M,3,4]`` or
        ``[S,M,3,4]`` as ``moved`` is shaped; ``out`` / ``out64`` are the tensors to write them to.  ``want64=False``: the float64 rows are
        not written (``transforms64`` is None).  No atomics: the same
        inputs give the same bits.  Needs no scene.  Only enqueues, on the current stream."""
        if not isinstance(nodes, torch.Tensor) or nodes.dim() != 2:
            raise ValueError("nodes must be a float32 device tensor [M,3]")
        m = int(nodes.shape[0])
        if not 1 <= m <= _capi.SAS_KNN_CROSS_MAX_NODES:
            raise ValueError(f"node_fit_rigid: m={m} out of [1, {_capi.SAS_KNN_CROSS_MAX_NODES}]")
        if not isinstance(moved, torch.Tensor) or moved.dim() not in (2, 3):
            raise ValueError(f"moved must be a float32 device tensor [{m},3] or [S,{m},3]")
        lead = tuple(moved.shape[:-2])
        steps = int(lead[0]) if lead else 1
        if steps < 1 or steps * m > _capi.SAS_NODES_FIT_MAX_LANES:
            raise ValueError(f"node_fit_rigid: {steps} time steps of {m} nodes: need 1 <= S and S * M <= {_capi.SAS_NODES_FIT_MAX_LANES}")
        kn = 0 if table is None else int(table.shape[1]) if isinstance(table, torch.Tensor) and table.dim() == 2 else -1
        if not 0 <= kn <= _capi.SAS_NODES_MAX_K:
            raise ValueError(f"node_fit_rigid: table must be [M,kn] with 0 <= kn <= {_capi.SAS_NODES_MAX_K}")
        g = self._node_array(nodes, torch.float32, (m, 3), "nodes")
        b = self._node_array(moved, torch.float32, lead + (m, 3), "moved")
        nb = self._node_array(table, torch.int32, (m, kn), "table") if kn > 0 else None
        shape = lead + (m, 3, 4)
        T32 = torch.empty(shape, dtype=torch.float32, device=self.device) if out is None else self._node_array(out, torch.float32, shape, "out")
        T64 = None
        if want64 or out64 is not None:
            T64 = torch.empty(shape, dtype=torch.float64, device=self.device) if out64 is None else self._node_array(out64, torch.float64, shape, "out64")
        rc = self._L.sas_nodes_fit_rigid(self._ctx, steps, m, _addr(g), _addr(b), kn, _addr(nb), _addr(T64), _addr(T32), self._stream())
        if rc != 0:
            self._check(rc, "sas_nodes_fit_rigid")
        return {"transforms": T32, "transforms64": T64}

    @_locked
    def read_order(self) -> torch.Tensor:
        """The resident scene's storage order (sas_scene_order): int32 ``[N]`` on the device, slot -> the caller's index, as
        ``storage_order(read_scene()["means"], group_id)`` gives it straight after an ``upload``, a ``densify`` or an ``mcmc_refine``.
        Blocking."""
        perm = torch.empty(self.n, dtype=torch.int32, device=self.device)
        torch.cuda.synchronize(self.device)   # (the allocator may hand out memory that work in flight still uses)
        self._check(self._L.sas_scene_order(self._ctx, _addr(perm)), "sas_scene_order")
        return perm

    @_locked
    def render_batch_host(self, viewmats: ArrayLike, Ks: ArrayLike, width: int, height: int,
                          background: Sequence[float] = (0.0, 0.0, 0.0), *, out: Optional[torch.Tensor] = None,
                          pose_sets: Optional[ArrayLike] = None, pose_set: Optional[Sequence[int]] = None) -> torch.Tensor:
        """C same-sized views as uint8 frames ON THE HOST (sas_render_batch_host): a pinned ``[C,H,W,3]`` uint8 CPU
        tensor, filled on the frames' own streams right behind the tile kernels -- what Door B's ``get_render``
        hands out (np.uint8 arrays), without a second round trip for the device-to-host copy.  ``out`` supplies the
        tensor (CPU, uint8, contiguous; pinned for speed); otherwise a pinned one comes from torch's caching host
        allocator, so a caller may keep what it gets."""
        keep, pV, pK, pbg, C, W, H = self._views(viewmats, Ks, background, width, height, True)   # (keep: the host arrays live to the end of this blocking call)
        out = self._host_frames(out, (C, H, W, 3))
        self._batch_call("sas_render_batch_host", C, pV, pK, pose_sets, pose_set, W, H, pbg, 0, out.data_ptr(), self._stream())
        return out

    @_locked
    def render_cameras_host(self, wxyz, position, fov: float, width: int, height: int,
                            background: Sequence[float] = (0.0, 0.0, 0.0), *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``render_batch_host`` from camera-to-world POSES (``wxyz [C,4]``, ``position [C,3]``, OpenCV axes) and a vertical
        field of view: the view matrices and intrinsics are computed inside the library (sas_render_cameras_host)."""
        q = np.ascontiguousarray(np.asarray(wxyz, dtype=np.float64).reshape(-1, 4))
        p = np.ascontiguousarray(np.asarray(position, dtype=np.float64).reshape(-1, 3))
        C, W, H = q.shape[0], int(width), int(height)
        bg = self._host_f32(background, 3)
        out = self._host_frames(out, (C, H, W, 3))
        stream = self._stream()
        rc = self._L.sas_render_cameras_host(self._ctx, C, q.ctypes.data, p.ctypes.data, float(fov), W, H, bg.ctypes.data, 0,
                                             out.data_ptr(), stream)
        if rc != 0:
            self._check(rc, "sas_render_cameras_host")
        return out

    @_locked
    def wait(self) -> None:
        self._check(self._L.sas_wait(self._ctx), "sas_wait")
        self._keep = []

    @_locked
    def frames_completed(self) -> Tuple[int, int]:
        """(submitted, completed) frame counts since creation (sas_frames_completed): frames
        ``0 .. completed-1`` are final and the current stream is ordered behind them."""
        sub, com = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.sas_frames_completed(self._ctx, ctypes.byref(sub), ctypes.byref(com)), "sas_frames_completed")
        return int(sub.value), int(com.value)

    # -- introspection ------------------------------------------------------------------------
    @_locked
    def stage_times(self) -> Dict[str, float]:
        ms = (ctypes.c_float * len(_capi.STAGE_NAMES))()
        self._check(self._L.sas_stage_times(self._ctx, ms, len(_capi.STAGE_NAMES)), "sas_stage_times")
        return dict(zip(_capi.STAGE_NAMES, [float(x) for x in ms]))

    @_locked
    def stage_time_means(self, reset: bool = True):
        """(mean ms per stage, frames) over the timed frames completed since the last reset."""
        ms = (ctypes.c_float * len(_capi.STAGE_NAMES))()
        nf = ctypes.c_int64(0)
        self._check(self._L.sas_stage_time_means(self._ctx, ms, len(_capi.STAGE_NAMES), ctypes.byref(nf), int(reset)),
                    "sas_stage_time_means")
        return dict(zip(_capi.STAGE_NAMES, [float(x) for x in ms])), int(nf.value)

    @_locked
    def stats(self) -> Dict[str, int]:
        st = (ctypes.c_int64 * len(_capi.STAT_NAMES))()
        self._check(self._L.sas_frame_stats(self._ctx, st, len(_capi.STAT_NAMES)), "sas_frame_stats")
        return dict(zip(_capi.STAT_NAMES, [int(x) for x in st]))

    @_locked
    def read_projection(self) -> Dict[str, np.ndarray]:
        n = self.n
        radii = np.zeros((n, 2), np.int32)
        means2d = np.zeros((n, 2), np.float32)
        depths = np.zeros((n,), np.float32)
        conics = np.zeros((n, 3), np.float32)
        colors = np.zeros((n, 3), np.float32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._L.sas_read_projection(self._ctx, p(radii), p(means2d), p(depths), p(conics), p(colors)),
                    "sas_read_projection")
        return dict(radii=radii, means2d=means2d, depths=depths, conics=conics, colors=colors)

    @_locked
    def read_tile_lists(self, tiles: int) -> Dict[str, np.ndarray]:
        m = self.stats()["n_isect"]
        off = np.zeros((tiles + 1,), np.int32)
        ids = np.zeros((max(m, 1),), np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._L.sas_read_tile_lists(self._ctx, p(off), p(ids), m), "sas_read_tile_lists")
        return dict(tile_offsets=off, sorted_ids=ids[:m])
