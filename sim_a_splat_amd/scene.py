"""Door B: the viser surface the Gym wrapper renders through, without viser or a browser.

Mirrors ``server.scene.add_gaussian_splats(...)`` handles with settable ``.wxyz/.position``
(sim_a_splat/splat/splat_handler.py:106-141, :283-288) and ``client.get_render(height, width,
wxyz, position)`` (sim_a_splat/env/splat/splat_env_wrapper.py:148-157).  All groups live in one
HIP scene; their poses go to the GPU as one [G,12] block per frame.
"""
from __future__ import annotations

import threading
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .poses import matrix_to_quat_wxyz, mv3, quat_wxyz_to_matrix, quats_wxyz_to_matrices
from .rasterizer import Rasterizer

DEFAULT_VERTICAL_FOV = float(np.deg2rad(75.0))   # the reference never passes a FOV; viser uses the client's


class GaussianSplatHandle:
    """What ``add_gaussian_splats`` returns: a group whose pose can be reassigned every step.  The scene keeps all
    group poses in one float32 ``[G,3,4]`` block (what goes to the GPU); a handle writes its row when it is assigned and
    reads it back when the poses were last set by the library's own link algebra (``SplatScene.set_link_poses``)."""

    def __init__(self, scene: "SplatScene", name: str, index: int, wxyz, position):
        self._scene, self.name, self.index = scene, name, index
        self._wxyz = np.asarray(wxyz, dtype=np.float64)
        self._position = np.asarray(position, dtype=np.float64)
        self._gen = scene._links_gen

    def _refresh(self) -> None:
        if self._gen != self._scene._links_gen:       # the block was rewritten by set_link_poses since
            row = self._scene._Rt[self.index].astype(np.float64)
            self._wxyz, self._position = matrix_to_quat_wxyz(row[:, :3]), row[:, 3].copy()
            self._gen = self._scene._links_gen

    def _write_row(self) -> None:
        sc = self._scene
        sc._Rt[self.index, :, :3] = quat_wxyz_to_matrix(self._wxyz)
        sc._Rt[self.index, :, 3] = self._position
        sc._poses_dirty = True

    @property
    def wxyz(self) -> np.ndarray:
        self._refresh()
        return self._wxyz

    @wxyz.setter
    def wxyz(self, v) -> None:
        with self._scene.lock:
            self._refresh()
            self._wxyz = np.asarray(v, dtype=np.float64)
            self._write_row()

    @property
    def position(self) -> np.ndarray:
        self._refresh()
        return self._position

    @position.setter
    def position(self, v) -> None:
        with self._scene.lock:
            self._refresh()
            self._position = np.asarray(v, dtype=np.float64)
            self._write_row()


class MeshHandle(GaussianSplatHandle):
    """What ``add_mesh_simple`` / ``add_mesh_trimesh`` return: a triangle mesh on a pose row of its own (DESIGN.md 3,
    "Meshes"), with the ``.wxyz`` / ``.position`` setters of a splat group.  Meshes and splat groups share the 256 rows."""


_NO_OWNER_APPLIED = object()   # SplatScene._link_owner_applied: the library's context holds nobody's link constants


class _Camera:
    def __init__(self):
        self.wxyz = np.array([1.0, 0.0, 0.0, 0.0])
        self.position = np.zeros(3)
        self.fov = DEFAULT_VERTICAL_FOV


def _camera_arrays(cam_poses):
    """Cameras ``[(wxyz, position), ...]`` as float64 arrays ``(q [C,4], p [C,3])``."""
    C = len(cam_poses)
    q, p = np.empty((C, 4), np.float64), np.empty((C, 3), np.float64)
    for c, (w, x) in enumerate(cam_poses):
        q[c], p[c] = w, x
    return q, p


class SplatScene:
    """Registered splat groups + the renderer (plays both ``server.scene`` and the client).

    Thread safety: ``lock`` (re-entrant) is held from the pose hand-over to the end of the render in every
    ``get_render*`` call, by ``add_gaussian_splats`` and by the handles' setters, so a viewer thread
    (``ViserBridge`` camera callbacks) and ``env.step`` on another thread (examples/demo_hw_splat.py:113-136 steps from
    a ROS2 callback) serialise on one scene instead of entering the C context together; a caller that assigns several
    handles as one update (``SplatHandler.draw_handler``) takes the lock around the whole update."""

    def __init__(self, device=0, background: Sequence[float] = (0.0, 0.0, 0.0)):
        self.lock = threading.RLock()
        self._raster = Rasterizer(device)
        self._groups: List[Dict[str, np.ndarray]] = []
        self._meshes: List[Dict[str, np.ndarray]] = []   # vertices (scaled), faces, per-face colours, pose row
        self._handles: List[GaussianSplatHandle] = []
        self._uploaded = False
        self._poses_dirty = True
        self._Rt = np.zeros((0, 3, 4), np.float32)     # all group poses, the block that goes to the GPU
        self._links_gen = 0                            # bumped when set_link_poses rewrites the block
        # constants of the link-pose algebra PER OWNER (a SplatHandler: its ICP similarity, forward kinematics, weld, groups).
        # The library's context holds one set; the scene applies the caller's before each use, so that two handlers on one
        # scene (two robots, `instance_uid`) never pose their links or cameras with each other's constants.
        self._link_consts: Dict[object, tuple] = {}
        self._link_owner_applied = _NO_OWNER_APPLIED
        self.background = tuple(background)
        self.mesh_ambient, self.mesh_diffuse = 0.4, 0.6   # mesh shading ("Meshes"); set before the first render
        self.camera = _Camera()
        self._deformable = None   # (handle, nodes, bind_kw) of bind_deformable: bound again whenever the scene is uploaded again
        self._driver = None       # the deform.NodeDriver of deform_positions, made on its first call; dropped by bind_deformable

    def _register(self, handle_class, name: str, wxyz, position):
        """(lock held)  A new handle on a pose row of its own, written into the block; the scene is uploaded again before the next frame."""
        if len(self._handles) >= 256:
            raise RuntimeError("at most 256 splat groups and meshes")
        h = handle_class(self, name, len(self._handles), wxyz, position)
        self._handles.append(h)
        self._Rt = np.concatenate([self._Rt, np.zeros((1, 3, 4), np.float32)], axis=0)
        h._write_row()
        self._uploaded = False
        return h

    def add_gaussian_splats(self, name: str, centers, covariances, rgbs, opacities, wxyz=(1.0, 0.0, 0.0, 0.0),
                            position=(0.0, 0.0, 0.0)) -> GaussianSplatHandle:
        c = np.ascontiguousarray(np.asarray(centers, dtype=np.float32).reshape(-1, 3))
        n = c.shape[0]
        group = dict(centers=c, covariances=np.asarray(covariances, dtype=np.float32).reshape(n, 3, 3),
                     rgbs=np.asarray(rgbs, dtype=np.float32).reshape(n, 3), opacities=np.asarray(opacities, dtype=np.float32).reshape(n))
        with self.lock:
            h = self._register(GaussianSplatHandle, name, wxyz, position)
            self._groups.append(dict(group, row=h.index))
        return h

    def add_mesh_simple(self, name: str, vertices, faces, color=(0.5, 0.5, 0.5), wxyz=(1.0, 0.0, 0.0, 0.0),
                        position=(0.0, 0.0, 0.0), scale: float = 1.0, vertex_normals=None, vertex_colors=None) -> MeshHandle:
        """viser's ``scene.add_mesh_simple``: ``vertices [V,3]`` (times ``scale``), ``faces [F,3]``, one colour (or ``[F,3]``).
        ``vertex_normals [V,3]`` (unit, mesh-local) make the mesh smooth-shaded ("Meshes", rule 2b), with
        ``vertex_colors [V,3]`` (0-1 or 0-255) interpolated over its triangles when given."""
        v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3) * float(scale)
        f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        col = np.asarray(color, dtype=np.float64)
        col = col / 255.0 if col.dtype.kind in "iu" or col.max(initial=0.0) > 1.0 else col
        col = np.broadcast_to(col.reshape(-1, 3) if col.size != 3 else col.reshape(1, 3), (f.shape[0], 3))
        if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
            raise ValueError(f"{name}: face index out of range")
        attr = {}
        for key, a in (("normals", vertex_normals), ("vcolors", vertex_colors)):
            if a is None:
                continue
            a = np.asarray(a, dtype=np.float64)
            if a.ndim != 2 or a.shape[0] != v.shape[0] or a.shape[1] < 3:
                raise ValueError(f"{name}: vertex {key} must be [V={v.shape[0]},3]")
            a = a[:, :3]
            if key == "vcolors" and (np.asarray(vertex_colors).dtype.kind in "iu" or a.max(initial=0.0) > 1.0):
                a = a / 255.0
            attr[key] = np.ascontiguousarray(a, dtype=np.float32)
        with self.lock:
            h = self._register(MeshHandle, name, wxyz, position)
            self._meshes.append(dict(row=h.index, vertices=v.astype(np.float32), faces=f.astype(np.int32),
                                     colors=np.ascontiguousarray(col, dtype=np.float32), **attr))
        return h

    def add_mesh_trimesh(self, name: str, mesh, scale: float = 1.0, wxyz=(1.0, 0.0, 0.0, 0.0),
                         position=(0.0, 0.0, 0.0), smooth: bool = False) -> MeshHandle:
        """viser's ``scene.add_mesh_trimesh``, duck-typed: ``mesh.vertices``, ``mesh.faces`` and, when present,
        ``mesh.visual.vertex_colors`` (RGB(A), 0-255 or 0-1) averaged over each face's three vertices.  ``smooth=True``: shaded
        from vertex normals (rule 2b) -- ``mesh.vertex_normals`` when present, else ``mesh_io.vertex_normals`` -- and the vertex
        colours are interpolated per vertex instead of averaged."""
        v = np.asarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
        f = np.asarray(mesh.faces, dtype=np.int64).reshape(-1, 3)
        vc = getattr(getattr(mesh, "visual", None), "vertex_colors", None)
        if vc is not None and len(vc) == len(v):
            vc = np.asarray(vc, dtype=np.float64)[:, :3]
            if vc.max(initial=0.0) > 1.0:
                vc = vc / 255.0
            color = vc[f].mean(axis=1)
        else:
            color, vc = (0.5, 0.5, 0.5), None
        if not smooth:
            return self.add_mesh_simple(name, v, f, color, wxyz=wxyz, position=position, scale=scale)
        vn = getattr(mesh, "vertex_normals", None)
        if vn is None or len(vn) != len(v):
            from .mesh_io import vertex_normals
            vn = vertex_normals(v, f)
        return self.add_mesh_simple(name, v, f, color, wxyz=wxyz, position=position, scale=scale, vertex_normals=vn, vertex_colors=vc)

    # -- the draw message's pose algebra inside the library (SplatHandler.draw_handler's fast path) ---------------
    def set_link_constants(self, scale: float, Ri, ti, Rfk, tfk, weld=None, groups=None, owner=None) -> None:
        """See ``Rasterizer.set_link_constants``; kept per ``owner`` (the handler they belong to) and applied to the
        library's context whenever that owner's poses or cameras are evaluated next."""
        with self.lock:
            self._link_consts[owner] = (float(scale), np.array(Ri, np.float64), np.array(ti, np.float64), np.array(Rfk, np.float64),
                                        np.array(tfk, np.float64), None if weld is None else np.array(weld, np.float64),
                                        None if groups is None else np.array(groups, np.int32))
            if self._link_owner_applied is owner or self._link_owner_applied == owner:
                self._link_owner_applied = _NO_OWNER_APPLIED   # re-apply on the next use

    def _apply_link_constants(self, owner) -> None:
        """(lock held, scene uploaded)  Make ``owner``'s constants the ones the library's context holds."""
        if owner not in self._link_consts:
            raise RuntimeError("set_link_constants first")
        if self._link_owner_applied is _NO_OWNER_APPLIED or self._link_owner_applied != owner:
            self._raster.set_link_constants(*self._link_consts[owner])
            self._link_owner_applied = owner

    def group_pose_rows(self) -> np.ndarray:
        """A copy of every group's current pose as float32 rows [G,12] (what goes to the GPU): the base of a per-env pose set."""
        with self.lock:
            return self._Rt.reshape(-1, 12).copy()

    def set_link_poses(self, q_msg, p_msg, owner=None) -> None:
        """The first k links' message poses -> their groups' poses (sas_set_link_poses: float64 in C, the arithmetic of
        ``poses.link_splat_poses`` + the quaternion round trip of the handles), with ``owner``'s constants; the other
        groups keep theirs."""
        with self.lock:
            if owner not in self._link_consts:
                raise RuntimeError("set_link_constants first")
            self._sync()                                    # scene + whatever the handles were assigned since
            self._apply_link_constants(owner)
            self._raster.set_link_poses(q_msg, p_msg, out=self._Rt.reshape(-1))
            self._links_gen += 1

    # -- deformable groups ("Deformation") ------------------------------------------
    def bind_deformable(self, handle: GaussianSplatHandle, nodes, **bind_kw) -> Dict[str, object]:
        """Make ``handle``'s splat group deformable: its Gaussians are bound to ``nodes [M,3]`` (the handle's LOCAL frame, the frame of
        ``add_gaussian_splats``' centers) as ``Rasterizer.bind_skin`` binds them (``k``, ``sigma``, ``max_distance``); every other group
        stays rigid.  The handle's ``.wxyz`` / ``.position`` still pose the deformed group.  One deformable group per scene.  Returns
        ``bind_skin``'s result."""
        with self.lock:
            if not isinstance(handle, GaussianSplatHandle) or isinstance(handle, MeshHandle) or handle._scene is not self:
                raise ValueError("bind_deformable: a splat-group handle of this scene is required")
            self._deformable = self._driver = None
            self._sync()
            res = self._raster.bind_skin(nodes, group=handle.index, **bind_kw)
            self._deformable = (handle, np.array(nodes, np.float32, copy=True), dict(bind_kw))
            return res

    def deform(self, node_transforms) -> None:
        """``Rasterizer.deform`` for the group of ``bind_deformable``: ``node_transforms [M,3,4]``, rest -> current in the handle's
        local frame.  The next ``get_render*`` shows it."""
        with self.lock:
            if self._deformable is None:
                raise RuntimeError("bind_deformable first")
            self._sync()
            self._raster.deform(node_transforms)

    def deform_positions(self, moved_nodes):
        """``deform`` from node POSITIONS: ``moved_nodes [M,3]`` (the handle's local frame; a float32 device tensor is read where it is),
        where the nodes of ``bind_deformable`` are now -- what a physics engine publishes.  A ``deform.NodeDriver`` over the stored nodes,
        made by the first call and kept until the next ``bind_deformable``, fits every node's rigid transform on the device and deforms
        the group; nothing is read back.  The handle's pose is applied on top, as for ``deform``.  Returns the transforms, the driver's
        float32 device tensor ``[M,3,4]``."""
        with self.lock:
            if self._deformable is None:
                raise RuntimeError("bind_deformable first")
            self._sync()
            if self._driver is None:
                from .deform import NodeDriver
                self._driver = NodeDriver(self._raster, self._deformable[1])
            return self._driver.drive(moved_nodes)

    def fit_deformation(self, images, height: int, width: int, cam_poses, fov: Optional[float] = None, iters: int = 200, masks=None, **kw):
        """How is the deformable group bent, given these pictures: ``deform.fit_node_transforms`` on the nodes of ``bind_deformable``, in the
        handle's local frame, so that the scene's frames from ``cam_poses [(wxyz, position), ...]`` look like ``images [C,H,W,3]`` (uint8,
        or float 0..1) over ``masks [C,H,W]``, with the views of ``get_renders``.  ``kw`` goes to ``fit_node_transforms`` (``start``,
        ``step``, ``factors``, ``rigidity_weight``; ``optimizer="device"`` keeps the nodes' twist update on the GPU, ``deform.NodeOptimizer``).  The scene is left deformed at the result, which the next ``get_render*`` shows; returns
        the ``NodeFit``.  The lock is held throughout; a scene with meshes is refused (the backward pass does not take occlusion by
        meshes)."""
        from .deform import fit_node_transforms
        V, K = self._views_and_Ks(int(height), int(width), *_camera_arrays(cam_poses), self._camera_or(fov=fov)[2])
        img = np.asarray(images.detach().cpu().numpy() if isinstance(images, torch.Tensor) else images)
        img = img.astype(np.float32) / 255.0 if img.dtype == np.uint8 else img.astype(np.float32)
        with self.lock:
            if self._deformable is None:
                raise RuntimeError("bind_deformable first")
            if self._meshes:
                raise RuntimeError("fit_deformation: the scene holds meshes, which the backward pass does not take")
            self._sync()
            return fit_node_transforms(self._raster, img, V, K, int(width), int(height), self._deformable[1], iters=iters, masks=masks,
                                       background=self.background, **kw)

    def fit_dynamic(self, frames, height: int, width: int, fov: Optional[float] = None, what=("means", "colors"), transforms=None,
                    iters: int = 100, **kw):
        """The deformable group's REST Gaussians from pictures of it in several bends: ``deform.fit_dynamic_scene`` on the nodes of
        ``bind_deformable``, in the handle's local frame.  ``frames``: one dict per time step with ``images [C,H,W,3]`` (uint8, or float
        0..1), ``cam_poses [(wxyz, position), ...]`` and optionally ``masks [C,H,W]``, with the views of ``get_renders``; ``transforms
        [S,M,3,4]``: the nodes' transforms of every time step.  ``what``: of ``means``, ``colors``, ``opacities`` (the covariances of a
        scene are fixed).  ``kw`` goes to ``fit_dynamic_scene`` (``fit_transforms``, ``lrs``, ``loss``, ``rigidity_weight``, ...; with ``fit_transforms``, ``optimizer="device"`` keeps the nodes' twist
        updates on the GPU).  Only
        the bound group is fitted (``bound_only=True``): every other group keeps its bits.  The fitted arrays replace the ones ``add_gaussian_splats`` was given, so
        a later upload keeps them; the scene is left deformed at the last time step.  Returns the ``DynamicFit``.  The lock is held
        throughout; a scene with meshes is refused."""
        from .deform import fit_dynamic_scene
        fov_ = self._camera_or(fov=fov)[2]
        packed = []
        for f in frames:
            V, K = self._views_and_Ks(int(height), int(width), *_camera_arrays(f["cam_poses"]), fov_)
            img = np.asarray(f["images"].detach().cpu().numpy() if isinstance(f["images"], torch.Tensor) else f["images"])
            img = img.astype(np.float32) / 255.0 if img.dtype == np.uint8 else img.astype(np.float32)
            packed.append(dict(images=img, viewmats=V, Ks=K, masks=f.get("masks")))
        with self.lock:
            if self._deformable is None:
                raise RuntimeError("bind_deformable first")
            if self._meshes:
                raise RuntimeError("fit_dynamic: the scene holds meshes, which the backward pass does not take")
            self._sync()
            r = self._raster
            res = fit_dynamic_scene(r, packed, self._deformable[1], what=what, transforms=transforms, iters=iters, background=self.background,
                                    bound_only=True, **kw)
            # the rest scene back into the groups' arrays: the skin is lifted for the read and bound again with the same entries
            skin = r.read_skin()
            r.clear_skin()
            rest = {k: v.cpu().numpy() for k, v in r.read_scene().items()}
            r.set_skin(skin["indices"], skin["weights"])
            r.deform(np.ascontiguousarray(res.transforms[-1].astype(np.float32)))
            at = 0
            for grp in self._groups:
                n = grp["centers"].shape[0]
                grp["centers"] = rest["means"][at:at + n].copy()
                grp["rgbs"] = rest["colors"][at:at + n].reshape(n, 3).copy()
                grp["opacities"] = rest["opacities"][at:at + n].copy()
                at += n
            return res

    # -- internals ---------------------------------------------------------------------------
    def _sync(self) -> None:
        if not self._uploaded:
            if not self._handles:
                z = np.zeros
                self._raster.upload(z((0, 3), np.float32), z((0,), np.float32), z((0, 3), np.float32),
                                    covariances=z((0, 6), np.float32), sh_degree=-1)
            else:
                # one pose row per handle (splat groups and meshes in creation order); group ids even for a single group
                # whenever meshes exist, so that a mesh's row is a group of the scene
                z = np.zeros
                cat = lambda k, shape: np.concatenate([g[k] for g in self._groups], axis=0) if self._groups else z(shape, np.float32)
                gid = np.concatenate([np.full(g["centers"].shape[0], g["row"], dtype=np.uint8) for g in self._groups]) \
                    if self._groups else np.zeros(0, np.uint8)
                self._raster.upload(cat("centers", (0, 3)), cat("opacities", (0,)), cat("rgbs", (0, 3)),
                                    covariances=cat("covariances", (0, 6)), sh_degree=-1, group_id=gid, n_groups=len(self._handles))
            if self._meshes:
                off = np.cumsum([0] + [m["vertices"].shape[0] for m in self._meshes])[:-1]
                # vertex attributes, when any mesh has them: zero normals keep the other meshes flat.  Vertex colours are one array
                # for the whole upload, so once any mesh has them a smooth mesh without gets its face colours per vertex
                attrs = {}
                if any("normals" in m for m in self._meshes):
                    attrs["vertex_normals"] = np.concatenate([m.get("normals", np.zeros_like(m["vertices"])) for m in self._meshes])
                    if any("vcolors" in m for m in self._meshes):
                        attrs["vertex_colors"] = np.concatenate([m["vcolors"] if "vcolors" in m else self._vertex_colours_of(m)
                                                                 for m in self._meshes])
                self._raster.upload_meshes(np.concatenate([m["vertices"] for m in self._meshes]),
                                           np.concatenate([m["faces"] + o for m, o in zip(self._meshes, off)]),
                                           np.concatenate([m["colors"] for m in self._meshes]),
                                           groups=np.concatenate([np.full(m["faces"].shape[0], m["row"], np.uint8) for m in self._meshes]),
                                           ambient=self.mesh_ambient, diffuse=self.mesh_diffuse, **attrs)
            self._uploaded = True
            self._poses_dirty = True
            self._link_owner_applied = _NO_OWNER_APPLIED    # a fresh upload: the context holds nobody's link constants
            if self._deformable is not None:                # ... and no skin
                h, nodes, kw = self._deformable
                self._raster.bind_skin(nodes, group=h.index, **kw)
        if self._poses_dirty and self._handles:
            self._raster.set_group_poses(self._Rt.reshape(-1, 12))
        self._poses_dirty = False

    @staticmethod
    def _vertex_colours_of(m) -> np.ndarray:
        """Per-vertex colours of a mesh registered without any, for an upload in which another mesh has them: each vertex takes
        the colour of the last face that uses it (exact for the one-colour meshes this serves; unused vertices 0.5 grey)."""
        vc = np.full(m["vertices"].shape, 0.5, np.float32)
        vc[m["faces"].reshape(-1)] = np.repeat(m["colors"], 3, axis=0)
        return vc

    @staticmethod
    def _view_and_K(height: int, width: int, wxyz, position, fov: float):
        """``_views_and_Ks`` of one camera: ([4,4], [3,3]) float32."""
        V, K = SplatScene._views_and_Ks(height, width, wxyz, position, fov)
        return V[0], K[0]

    @staticmethod
    def _views_and_Ks(height: int, width: int, wxyz: np.ndarray, position: np.ndarray, fov: float):
        """World-to-camera matrices and intrinsics of C cameras ``wxyz [C,4]``, ``position [C,3]``: ([C,4,4], [C,3,3]) float32."""
        R = quats_wxyz_to_matrices(wxyz)                   # camera-to-world, OpenCV axes (+z forward, +y down)
        C = R.shape[0]
        V = np.zeros((C, 4, 4))
        Rt = np.transpose(R, (0, 2, 1))
        V[:, :3, :3] = Rt
        V[:, :3, 3] = -mv3(Rt, np.asarray(position, dtype=np.float64).reshape(C, 3))
        V[:, 3, 3] = 1.0
        f = 0.5 * height / np.tan(0.5 * fov)               # vertical FOV, square pixels
        K = np.array([[f, 0, 0.5 * width], [0, f, 0.5 * height], [0, 0, 1]])
        return V.astype(np.float32), np.broadcast_to(K.astype(np.float32), (C, 3, 3)).copy()

    # -- client side ---------------------------------------------------------------------------
    def _camera_or(self, wxyz=None, position=None, fov: Optional[float] = None):
        """(wxyz, position, fov) with the client's own camera standing in for whatever is None."""
        cam = self.camera
        return cam.wxyz if wxyz is None else wxyz, cam.position if position is None else position, cam.fov if fov is None else float(fov)

    def get_render(self, height: int, width: int, wxyz=None, position=None, fov: Optional[float] = None) -> np.ndarray:
        """uint8 [H,W,3] frame from a camera pose (camera-to-world, OpenCV axes)."""
        wxyz, position, f = self._camera_or(wxyz, position, fov)
        with self.lock:
            self._sync()
            # view matrix and intrinsics inside the library (sas_camera_matrices: the arithmetic of _view_and_K)
            return self._raster.render_cameras_host(wxyz, position, f, int(width), int(height), self.background).numpy()[0]

    def get_renders(self, height: int, width: int, cam_poses, fov: Optional[float] = None) -> np.ndarray:
        """uint8 [C,H,W,3] for C same-sized cameras ``[(wxyz, position), ...]`` in one batched call."""
        q, p = _camera_arrays(cam_poses)
        f = self._camera_or(fov=fov)[2]
        with self.lock:
            self._sync()
            # view matrices and intrinsics inside the library (sas_camera_matrices: the arithmetic of _views_and_Ks); frames
            # land in pinned host memory on the frames' own streams (sas_render_batch_host): no second round trip
            return self._raster.render_cameras_host(q, p, f, int(width), int(height), self.background).numpy()

    def get_renders_posed(self, height: int, width: int, cam_poses, pose_sets, pose_set, fov: Optional[float] = None,
                          out: Optional[torch.Tensor] = None, device_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [C,H,W,3] (pinned host tensor) for C same-sized cameras of SEVERAL envs in one call: view v is rendered
        with the group poses ``pose_sets[pose_set[v]]`` ([S,G,12] float32; vectorised envs, sas_render_batch_host_posed)
        instead of the scene's current ones; ``out`` supplies the tensor.  ``device_out`` (a uint8 [C,H,W,3] tensor on the
        scene's GPU) keeps the frames ON THE DEVICE instead (sas_render_batch_posed): what a multi-GPU rollout gathers
        over RCCL without the frames ever visiting the host on the way."""
        V, K = self._views_and_Ks(int(height), int(width), *_camera_arrays(cam_poses), self._camera_or(fov=fov)[2])
        with self.lock:
            self._sync()
            if device_out is not None:
                return self._raster.render_batch(V, K, int(width), int(height), self.background, want=("rgb8",), out={"rgb8": device_out},
                                                 pose_sets=pose_sets, pose_set=pose_set)["rgb8"]
            return self._raster.render_batch_host(V, K, int(width), int(height), self.background, out=out, pose_sets=pose_sets, pose_set=pose_set)

    def attached_frame(self, q_link, p_link, local_xyz, owner=None):
        """(wxyz, xyz) of a camera riding on a link, with the similarity of ``owner``'s ``set_link_constants`` (sas_link_attached_frame)."""
        with self.lock:
            if owner not in self._link_consts:
                raise RuntimeError("set_link_constants first")
            self._sync()
            self._apply_link_constants(owner)
            return self._raster.link_attached_frame(q_link, p_link, local_xyz)

    def get_render_float(self, height: int, width: int, wxyz, position, fov: Optional[float] = None,
                         mesh_surface: bool = False) -> Dict[str, torch.Tensor]:
        """float32 device tensors ``rgb`` / ``alpha`` / ``depth``; ``mesh_surface=True``: alpha and depth of the whole scene, the
        meshes' surfaces included (``Rasterizer.render``)."""
        V, K = self._view_and_K(int(height), int(width), *self._camera_or(wxyz, position, fov))
        with self.lock:
            self._sync()
            return self._raster.render(V, K, int(width), int(height), self.background, want=("rgb", "alpha", "depth"),
                                       mesh_surface=mesh_surface)

    def row_names(self) -> List[str]:
        """The handles' names by pose row: ``row_names()[label]`` names what a pixel of ``get_segmentation`` shows (splat groups
        and meshes share one row numbering, in creation order)."""
        with self.lock:
            return [h.name for h in self._handles]

    def get_segmentation(self, height: int, width: int, wxyz=None, position=None, fov: Optional[float] = None,
                         min_alpha: float = 0.5) -> Dict[str, torch.Tensor]:
        """Which handle each pixel shows (``Rasterizer.render_group_masks``): ``labels [H,W]`` uint8, the pose-row index of the
        splat group or mesh (255: none, alpha < min_alpha), ``weights [H,W,rows]`` and ``alpha [H,W,1]`` (a mesh counts as
        opaque).  Device tensors."""
        V, K = self._view_and_K(int(height), int(width), *self._camera_or(wxyz, position, fov))
        with self.lock:
            if not self._handles:
                raise RuntimeError("get_segmentation needs at least one splat group or mesh")
            self._sync()
            return self._raster.render_group_masks(V, K, int(width), int(height), min_alpha=min_alpha)

    def get_observations(self, height: int, width: int, cam_poses, fov: Optional[float] = None, pose_sets=None, pose_set=None,
                         min_alpha: float = 0.5, want: Sequence[str] = ("labels",)) -> Dict[str, torch.Tensor]:
        """Label frames of C same-sized cameras ``[(wxyz, position), ...]`` in one call (``Rasterizer.render_batch_labels``):
        ``labels [C,H,W]`` uint8 and any of ``rgb8 [C,H,W,3]`` / ``depth [C,H,W,1]`` / ``alpha`` / ``rgb`` named in ``want``, device
        tensors; meshes count as surfaces (depth closes on them, alpha is 1).  ``pose_sets`` / ``pose_set``: per-view pose sets."""
        V, K = self._views_and_Ks(int(height), int(width), *_camera_arrays(cam_poses), self._camera_or(fov=fov)[2])
        with self.lock:
            if not self._handles:
                raise RuntimeError("label frames need at least one splat group or mesh")
            self._sync()
            return self._raster.render_batch_labels(V, K, int(width), int(height), self.background, min_alpha=min_alpha, want=tuple(want),
                                                    pose_sets=pose_sets, pose_set=pose_set)

    def _keep_rows(self, keep) -> Optional[List[int]]:
        """``keep`` of ``get_point_clouds`` -- row names (``row_names()``) or row indices -- as row indices; None stays None."""
        if keep is None:
            return None
        names = self.row_names()
        rows = []
        for k in keep:
            if isinstance(k, str):
                if k not in names:
                    raise ValueError(f"keep: no row named {k!r} (rows: {names})")
                rows.append(names.index(k))
            else:
                if not 0 <= int(k) < len(names):
                    raise ValueError(f"keep: row {int(k)} out of [0,{len(names)})")
                rows.append(int(k))
        return rows

    def get_point_clouds(self, height: int, width: int, cam_poses, n_points: int, *, bounds=None, voxel_size: float = 0.0,
                         stride: int = 1, keep=None, frame=None, pose_sets=None, pose_set=None, clouds=None, n_clouds: int = 1,
                         fov: Optional[float] = None, min_alpha: float = 0.5) -> Dict[str, torch.Tensor]:
        """Fixed-size point clouds of C same-sized cameras ``[(wxyz, position), ...]``: one label-frame call
        (``Rasterizer.render_batch_labels`` with rgb8 and depth) and one sampling call (``Rasterizer.sample_point_cloud``) on its
        device outputs -- nothing visits the host.  ``n_points`` per cloud by farthest-point sampling, in the world frame or,
        with ``frame`` (4x4, world to output frame), beyond it; ``bounds`` ``(lo[3], hi[3])``, ``voxel_size`` and ``stride`` thin
        the pixels first; ``keep``: the rows whose pixels count, by name (``row_names()``) or index.  ``pose_sets`` /
        ``pose_set``: per-view pose sets; ``clouds [C]`` / ``n_clouds``: the cloud each camera feeds (vectorised envs: one cloud
        per env).  Returns device tensors ``points [E,K,3]``, ``index [E,K]``, ``colors [E,K,3]``, ``labels [E,K]`` (row
        indices; 255 padding), ``count [E]``, and ``frames``, the label-frame call's own outputs."""
        V, K = self._views_and_Ks(int(height), int(width), *_camera_arrays(cam_poses), self._camera_or(fov=fov)[2])
        with self.lock:
            if not self._handles:
                raise RuntimeError("point clouds need at least one splat group or mesh")
            rows = self._keep_rows(keep)
            self._sync()
            o = self._raster.render_batch_labels(V, K, int(width), int(height), self.background, min_alpha=min_alpha,
                                                 want=("rgb8", "depth"), pose_sets=pose_sets, pose_set=pose_set)
            res = self._raster.sample_point_cloud(o["depth"], V, K, int(width), int(height), int(n_points), rgb8=o["rgb8"],
                                                  labels=o["labels"], keep_labels=rows, bounds=bounds, voxel_size=voxel_size,
                                                  stride=stride, frame=frame, clouds=clouds, n_clouds=n_clouds)
            res["frames"] = o
            return res

    def fuse_views(self, volume, height: int, width: int, cam_poses, *, keep=None, fov: Optional[float] = None, frame=None,
                   min_alpha: float = 0.5, **fuse_kw) -> Dict[str, torch.Tensor]:
        """Integrate what C same-sized cameras ``[(wxyz, position), ...]`` see into ``volume`` (``reconstruct.TsdfVolume``): one
        label-frame call (``Rasterizer.render_batch_labels`` with depth and rgb8, the background's depth filled) and one fusion
        call (``Rasterizer.fuse_depth``) on its device outputs -- nothing visits the host.  ``keep``: the rows that are the surface,
        by name (``row_names()``) or index; pixels of other rows, and the filled background, carve the free space in front of
        themselves -- which is what closes the surface behind the object's silhouette.  ``frame`` (4x4, world to volume frame) and
        ``fuse_kw`` (``trunc``, ``near``, ``max_weight``) go to ``fuse_depth``.  Returns the label-frame call's outputs."""
        V, K = self._views_and_Ks(int(height), int(width), *_camera_arrays(cam_poses), self._camera_or(fov=fov)[2])
        with self.lock:
            if not self._handles:
                raise RuntimeError("fusion needs at least one splat group or mesh")
            rows = self._keep_rows(keep)
            self._sync()
            o = self._raster.render_batch_labels(V, K, int(width), int(height), self.background, min_alpha=min_alpha,
                                                 want=("depth", "rgb8"), depth_fill_max=True)
            self._raster.fuse_depth(volume, o["depth"], V, K, int(width), int(height), rgb8=o["rgb8"], labels=o["labels"],
                                    keep_labels=rows, frame=frame, pixel_centre=0.5, **fuse_kw)
            return o

    def get_segmentations(self, height: int, width: int, cam_poses, fov: Optional[float] = None, pose_sets=None, pose_set=None,
                          min_alpha: float = 0.5) -> torch.Tensor:
        """``get_segmentation``'s ``labels`` for C same-sized cameras ``[(wxyz, position), ...]`` in one call: uint8 ``[C,H,W]`` on the
        device, the pose-row index each pixel shows (``row_names()``; 255: none).  ``pose_sets [S,rows,12]`` + ``pose_set [C]``:
        camera c sees the scene under ``pose_sets[pose_set[c]]`` (vectorised envs); the scene's own poses are not touched."""
        return self.get_observations(height, width, cam_poses, fov, pose_sets, pose_set, min_alpha)["labels"]

    def refine_handle_poses(self, handles, images, height: int, width: int, cam_poses, fov: Optional[float] = None, iters: int = 200,
                            masks=None):
        """Where are these groups, given these pictures: refine the poses of ``handles`` (up to 32 splat-group handles) so that the
        scene's frames from ``cam_poses [(wxyz, position), ...]`` look like ``images [C,H,W,3]`` (uint8, or float 0..1) over ``masks
        [C,H,W]`` -- ``register.refine_group_poses`` on the handles' pose rows, each turning about the posed centroid of its centres,
        with the views of ``get_renders``.  On return the handles' ``wxyz`` (a unit quaternion) and ``position`` hold the refined poses,
        and the result (``GroupPoseRefinement``) the whole block.  The lock is held throughout; a scene with meshes is refused (the
        backward pass does not take occlusion by meshes)."""
        from .register import refine_group_poses
        hs = list(handles)
        V, K = self._views_and_Ks(int(height), int(width), *_camera_arrays(cam_poses), self._camera_or(fov=fov)[2])
        img = np.asarray(images.detach().cpu().numpy() if isinstance(images, torch.Tensor) else images)
        img = img.astype(np.float32) / 255.0 if img.dtype == np.uint8 else img.astype(np.float32)
        with self.lock:
            by_row = {g["row"]: g for g in self._groups}
            for h in hs:
                if h._scene is not self or h.index not in by_row:
                    raise ValueError(f"refine_handle_poses: {getattr(h, 'name', h)!r} is not a splat group of this scene")
            self._sync()
            pivots = np.stack([mv3(self._Rt[h.index, :, :3].astype(np.float64), by_row[h.index]["centers"].astype(np.float64)).mean(axis=0)
                               + self._Rt[h.index, :, 3] for h in hs])
            res = refine_group_poses(self._raster, img, V, K, int(width), int(height), [h.index for h in hs], iters=iters, masks=masks,
                                     pivots=pivots, background=self.background)
            for h in hs:   # through a unit quaternion, as the setters do; the block is rewritten from the handles
                h._refresh()
                h._wxyz = np.asarray(matrix_to_quat_wxyz(res.poses[h.index, :, :3]), np.float64)
                h._wxyz = h._wxyz / np.linalg.norm(h._wxyz)
                h._position = res.poses[h.index, :, 3].copy()
                h._write_row()
            return res

    def close(self) -> None:
        with self.lock:
            self._raster.close()
