"""The dynamic-scene front end of the Gym wrapper on the HIP rasterizer.

``SplatHandler`` (same constructor arguments as sim_a_splat/splat/splat_handler.py:22-38) partitions the
Gaussians into per-link groups plus the static rest (:104-143), turns Drake draw messages into group
poses (:227-314) and renders camera lists (:334-346).  ``CameraRig`` holds the camera dictionary logic
of ``SplatEnvWrapper._configure_cameras/render/_get_obs`` (splat_env_wrapper.py:33-65, :105-159); the
wrapper itself is ``sim_a_splat_amd.env_wrapper.SplatEnvWrapper``.  Nothing here imports viser, pydrake
or gymnasium: messages, poses and the weld frame are duck-typed.
"""
from __future__ import annotations

import logging
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import poses
from .scene import SplatScene


def aabb_mask(means, bounds) -> np.ndarray:
    """Axis-aligned bounding-box mask of ``_load_saved_splats`` (splat_handler.py:91-97): ``bounds`` is
    [3,2] (min, max per axis) or None for "keep everything" (the reference passes None)."""
    means = np.asarray(means)
    if bounds is None:
        return np.ones(means.shape[0], dtype=bool)
    b = np.asarray(bounds, dtype=means.dtype)
    return np.all((means - b[:, 0] >= 0) & (b[:, 1] - means >= 0), axis=-1)


def _translation_of(x) -> np.ndarray:
    """Translation of the robot weld frame: a 3-vector, or an object with ``.translation()`` (pydrake
    RigidTransform in the reference, splat_handler.py:229; only identity rotations are supported there)."""
    if x is None:
        return np.zeros(3)
    if hasattr(x, "translation"):
        t = x.translation() if callable(x.translation) else x.translation
        return np.asarray(t, dtype=np.float64).reshape(3)
    return np.asarray(x, dtype=np.float64).reshape(3)


def _entries(msg, robot_num: int) -> List[int]:
    """The draw message's entries of one ``robot_num``, in message order."""
    rn = msg.robot_num
    return [i for i in range(msg.num_links) if rn[i] == robot_num]


def _cameras(chs, cam_poses) -> List[Tuple[np.ndarray, np.ndarray]]:
    """``cam_poses`` (SE3-like objects or pairs; None: the client's own camera) as ``(wxyz, xyz)`` pairs."""
    if cam_poses is None:
        cam_poses = [(chs.camera.wxyz, chs.camera.position)]
    return [poses.pose_wxyz_xyz(p) for p in cam_poses]


def _by_size(render_size, n: int) -> Dict[Tuple[int, int], List[int]]:
    """``{(H, W): [cameras of that size]}`` over the first ``n`` cameras, sizes in order of first appearance: one batch each."""
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, s in enumerate(render_size[:n]):
        groups.setdefault((int(s[0]), int(s[1])), []).append(i)
    return groups


def _checked_modes(modes, what: str = "observation modes") -> Tuple[str, ...]:
    """Observation modes as a tuple; ValueError (naming them ``what``) on one that is not among ``SplatHandler.OBS_MODES``."""
    modes = tuple(modes)
    bad = [m for m in modes if m not in SplatHandler.OBS_MODES]
    if bad:
        raise ValueError(f"unknown {what} {bad}: choose from {SplatHandler.OBS_MODES}")
    return modes


TASK_MESH_COLOR = (0.956, 0.396, 0.365)   # splat_handler.py:205


ROBOT_MESH_DEFAULT_COLOR = (0.5, 0.5, 0.5)   # a visual without a material colour


def robot_visual_meshes(robot, robot_description_dir: str, package_name: str, urdf_dir=None) -> list:
    """The robot's visual meshes as ``_add_robot_meshes`` collects them (splat_handler.py:145-173): for every link in URDF
    order, every visual with a mesh -> ``(vertices, faces, rgb)``.  ``package://{package_name}`` in a mesh filename is replaced
    by ``robot_description_dir`` (the reference does so in the URDF text); any other relative filename is taken relative to the
    URDF's directory.  rgb: the visual's material colour, (0.5, 0.5, 0.5) without one.  As in the reference, neither the
    visual's ``<origin>`` nor the mesh ``scale`` is applied to the vertices."""
    from pathlib import Path
    from . import mesh_io
    out = []
    for link in robot.links:
        for vis in robot.visuals[link]:
            if not vis.mesh:
                continue
            fn = vis.mesh.replace(f"package://{package_name}", robot_description_dir)
            if fn.startswith("file://"):
                fn = fn[len("file://"):]
            path = Path(fn)
            if not path.is_absolute() and urdf_dir is not None:
                path = Path(urdf_dir) / path
            v, f = mesh_io.load_mesh(path)
            out.append((v, f, ROBOT_MESH_DEFAULT_COLOR if vis.color is None else tuple(float(x) for x in vis.color)))
    return out


def _mesh_arrays(meshes, task_assets_path=None, task_assets_name=None, robot_meshes=None) -> Dict[str, object]:
    """``meshes`` as names or arrays -> ``{"task": (vertices, faces), "robot": [(vertices, faces, rgb), ...]}`` (mesh-local,
    unscaled).  ``robot_meshes``: a callable that reads the URDF's visuals (the path constructor's), for ``"robot"`` by name."""
    from . import mesh_io
    out: Dict[str, object] = {}
    items = meshes.items() if isinstance(meshes, dict) else ((m, None) for m in (meshes or ()))
    for name, val in items:
        if name == "robot":
            if val is None:
                if robot_meshes is None:
                    raise NotImplementedError("meshes=('robot',) by name reads the URDF's visuals: the path constructor does; from arrays "
                                              "pass them, {'robot': [(vertices, faces, rgb), ...]}")
                val = robot_meshes()
            out["robot"] = [(np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3),
                             tuple(float(x) for x in np.asarray(rgb, np.float64).reshape(-1)[:3])) for v, f, rgb in val]
            continue
        if name != "task":
            raise ValueError(f"unknown mesh {name!r}: 'task', 'robot'")
        if val is None:
            if not task_assets_name:
                raise ValueError("meshes=('task',) needs task_assets_path and task_assets_name")
            val = mesh_io.load_mesh(f"{task_assets_path}/{task_assets_name}")
        v, f = val
        out["task"] = (np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3))
    return out


class SplatHandler:
    """``SplatHandler(splat_assets_path, match_object_name, splat_config_name, package_path, package_name,
    urdf_name, task_assets_path=None, task_assets_name=None, sim_robot_weld_frame_transform=..., server=None)``
    -- the reference's constructor (splat_handler.py:22-60) with the same argument meaning:

    * masks, ICP similarity and mask-time joint configuration from ``{splat_assets_path}/masks/{match_object_name}/``;
    * Gaussians from ``{splat_assets_path}/splatfacto/{splat_config_name}`` (``GSplatLoader.from_path``);
    * URDF ``{package_path}/{package_name}urdf/{urdf_name}`` (the reference concatenates exactly so, :52,148)
      for the visual-mesh forward kinematics;
    * ``server``: where the reference takes a viser server, this takes the object that plays ``server.scene`` +
      the client, a ``SplatScene`` (created on ``device`` when None);
    * ``meshes`` (not in the reference, default ``()``: splats only): ``"task"`` composites the task object
      ``{task_assets_path}/{task_assets_name}`` into every frame, in the reference's colour (0.956, 0.396, 0.365), scaled by the
      ICP scale and posed by ``draw_handler`` as at :296-314 (``_add_task_meshes``, :199-219).  ``"robot"`` composites the
      robot's URDF visual meshes (``_add_robot_meshes``, :145-197): welded, smooth-shaded from computed vertex normals in the
      visual's material colour ("Meshes", rule 2b), one mesh ``{uid}/mesh_robot/link{ii}`` each, posed as at :238-263.

    ``SplatHandler.from_arrays`` builds the same object from arrays already in memory."""

    task_mesh_frame_handle = None    # a handler has no meshes until _setup registers some
    mesh_frame_handles = ()

    def __init__(self, splat_assets_path: str, match_object_name: str, splat_config_name: str, package_path: str,
                 package_name: str, urdf_name: str, task_assets_path: Optional[str] = None,
                 task_assets_name: Optional[str] = None, sim_robot_weld_frame_transform=None, server: Optional[SplatScene] = None,
                 *, device=0, bounds=None, meshes=()):
        from pathlib import Path
        from . import urdf_fk
        from .covariance import GSplatLoader
        masks_dir = Path(f"{splat_assets_path}/masks/{match_object_name}/").resolve()
        loader = GSplatLoader.from_path(Path(f"{splat_assets_path}/splatfacto/{splat_config_name}").resolve())
        robot_description_dir = package_path + "/" + package_name
        urdf_path = Path(robot_description_dir + f"urdf/{urdf_name}")
        robot = urdf_fk.load(urdf_path)
        meshes = _mesh_arrays(meshes, task_assets_path, task_assets_name,
                              robot_meshes=lambda: robot_visual_meshes(robot, robot_description_dir, package_name, urdf_path.parent))
        self._setup(*self._load_assets(loader, masks_dir, robot, bounds),
                    instance_uid=match_object_name, weld=sim_robot_weld_frame_transform, scene=server, device=device, meshes=meshes)
        self.masks_dir = str(masks_dir)
        self.robot_description_dir = robot_description_dir
        self.rbt_drake_namespace = f"plant::{urdf_name.split('.')[0]}::"                       # :58-60
        self.blk_drake_namespace = f"plant::{task_assets_name.split('.')[0]}::" if task_assets_name else None

    @classmethod
    def from_arrays(cls, means, covs, colors, opacities, link_masks: Dict[str, np.ndarray], icp_transformation: np.ndarray,
                    fk_transforms: Sequence[np.ndarray], instance_uid: str = "robot", robot_num: int = 3,
                    weld_translation=(0.0, 0.0, 0.0), scene: Optional[SplatScene] = None, device=0, meshes=(),
                    task_assets_path: Optional[str] = None, task_assets_name: Optional[str] = None) -> "SplatHandler":
        """The same handler from arrays: Gaussians [N,...], the per-link boolean masks ``link0..``, the 4x4 ICP
        similarity and one 4x4 forward-kinematics pose per visual mesh at the mask-time joint configuration.
        ``meshes``: names (``"task"``: read from ``task_assets_path/task_assets_name``) or arrays,
        ``{"task": (vertices [V,3], faces [F,3]), "robot": [(vertices, faces, rgb), ...]}`` (the robot's visual meshes in
        ``robot_visual_meshes`` order; by name they need the URDF, i.e. the path constructor)."""
        self = cls.__new__(cls)
        self._setup(means, covs, colors, opacities, link_masks, icp_transformation, fk_transforms, instance_uid=instance_uid,
                    weld=weld_translation, scene=scene, device=device, robot_num=robot_num,
                    meshes=_mesh_arrays(meshes, task_assets_path, task_assets_name))
        return self

    def _setup(self, means, covs, colors, opacities, link_masks, icp_transformation, fk_transforms, *, instance_uid, weld,
               scene, device, robot_num: int = 3, meshes=None) -> None:
        self.scene = scene if scene is not None else SplatScene(device)
        self.server = self.scene                               # the reference's name for it (close(), clients)
        self.instance_uid = instance_uid
        self.rbt_idx, self.blk_idx = robot_num, 2              # splat_handler.py:58
        self.weld_translation = _translation_of(weld)
        self.scale_factor, self.Ri, self.ti = poses.decompose_icp(icp_transformation)
        self.fk = [(np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3]) for T in fk_transforms]
        self._fkR = np.stack([R for R, _ in self.fk]) if self.fk else np.zeros((0, 3, 3))
        self._fkt = np.stack([t for _, t in self.fk]) if self.fk else np.zeros((0, 3))
        means, covs = np.asarray(means, np.float32), np.asarray(covs, np.float32)
        colors, opacities = np.asarray(colors, np.float32), np.asarray(opacities, np.float32).reshape(-1)
        self.means, self.covs, self.colors, self.opacities = means, covs, colors, opacities   # :99-102
        n = means.shape[0]
        self.robot_splat_idxs = np.zeros(n, dtype=bool)
        self.splat_links_handler = []
        for ii in range(len(link_masks)):                      # link0..linkK-1 in order (:124-143)
            idxs = np.asarray(link_masks[f"link{ii}"], dtype=bool)
            self.splat_links_handler.append(self.scene.add_gaussian_splats(
                f"{instance_uid}/splat_robot/link{ii}", means[idxs], covs[idxs], colors[idxs], opacities[idxs]))
            self.robot_splat_idxs |= idxs
        rest = ~self.robot_splat_idxs                          # "/scene_ohne_robot" (:112-119)
        self.scene_handle = self.scene.add_gaussian_splats("/scene_ohne_robot", means[rest], covs[rest], colors[rest],
                                                           opacities[rest])
        # task mesh (_add_task_meshes, :199-219): vertices scaled by the ICP scale, the reference's colour, a pose row of its own
        self.task_mesh_frame_handle = None
        if meshes and "task" in meshes:
            v, f = meshes["task"]
            self.task_mesh_frame_handle = self.scene.add_mesh_simple(f"{instance_uid}/mesh_task/task", v, f, TASK_MESH_COLOR,
                                                                     scale=self.scale_factor)
        # robot meshes (_add_robot_meshes, :175-197): one smooth mesh per visual, welded (an STL shares no vertex), with computed
        # vertex normals, in the visual's material colour, vertices times the ICP scale
        self.mesh_frame_handles = []
        if meshes and meshes.get("robot"):
            from . import mesh_io
            for ii, (v, f, rgb) in enumerate(meshes["robot"]):
                v, f = mesh_io.weld(v, f)
                self.mesh_frame_handles.append(self.scene.add_mesh_simple(
                    f"{instance_uid}/mesh_robot/link{ii}", v, f, rgb, scale=self.scale_factor, vertex_normals=mesh_io.vertex_normals(v, f)))
        # the draw message's pose algebra runs inside the library when the scene offers it (sas_set_link_poses)
        self._k_fast = min(len(self.fk), 7, len(self.splat_links_handler))
        self._fast = hasattr(self.scene, "set_link_poses") and self._k_fast > 0
        if self._fast:
            # kept by the scene under THIS handler's key: a second handler on the same scene has constants of its own
            self.scene.set_link_constants(self.scale_factor, self.Ri, self.ti, self._fkR[:self._k_fast], self._fkt[:self._k_fast],
                                          self.weld_translation, [h.index for h in self.splat_links_handler[:self._k_fast]], owner=id(self))

    @classmethod
    def from_assets(cls, loader, masks_dir, urdf_path, bounds=None, **kw) -> "SplatHandler":
        """Like the path constructor, with the Gaussians already loaded (a ``GSplatLoader``) and the masks
        directory / URDF file given directly; ``bounds`` is the AABB crop of ``_load_saved_splats``."""
        from . import urdf_fk
        return cls.from_arrays(*cls._load_assets(loader, masks_dir, urdf_fk.load(urdf_path), bounds), **kw)

    @staticmethod
    def _load_assets(loader, masks_dir, robot, bounds) -> tuple:
        """What a handler reads from disk, as the leading arguments of ``from_arrays``: the loader's Gaussians and the link masks
        of ``masks_dir`` cropped to ``bounds``, the ICP similarity, and ``robot``'s visual-mesh forward kinematics at the mask-time
        joint configuration."""
        from pathlib import Path
        from . import io, urdf_fk
        d = Path(masks_dir)
        mfile = d / "link_masks_global_dict.npz"
        masks = io.load_link_masks(mfile if mfile.exists() else d / "link_masks_global_dict.npy")
        icp = io.load_icp_transformation(d / "icp_transformation.npy")
        fk = urdf_fk.visual_mesh_fk(robot, io.load_joint_config(d / "joint_config.npy"))
        keep = aabb_mask(loader.means.cpu().numpy(), bounds)
        arr = lambda t: t.cpu().numpy()[keep]
        masks = {k: np.asarray(v, dtype=bool)[keep] for k, v in masks.items()}
        return arr(loader.means), arr(loader.covs), arr(loader.colors), arr(loader.opacities), masks, icp, fk

    def mesh_pose_rows(self, msg) -> Tuple[np.ndarray, np.ndarray]:
        """The pose rows ``draw_handler(msg)`` gives this handler's meshes, WITHOUT touching the scene: ``(rows [m], [m,12]
        float32)``.  Task mesh: the last entry with ``robot_num == blk_idx``, ``icp o SE3(q/|q|, p s)`` in float64 (:296-314),
        through the handle's quaternion as ``draw_handler`` assigns it.  Robot meshes: the k-th entry with ``robot_num ==
        rbt_idx`` poses the k-th mesh, ``icp o SE3(q/|q|, (p + weld) s)`` (:238-263); surplus entries are ignored."""
        found = list(self._mesh_entries(msg))
        rows = np.zeros((len(found), 3, 4), np.float32)
        for k, (_, wxyz, t) in enumerate(found):
            rows[k, :, :3] = poses.quat_wxyz_to_matrix(wxyz)
            rows[k, :, 3] = t
        return np.array([h.index for h, _, _ in found], np.int64), rows.reshape(len(found), 12)

    def _mesh_entries(self, msg):
        """``(handle, wxyz, t)`` for every mesh the message poses: the task mesh at its last ``blk_idx`` entry (the reference assigns
        every one in turn), the k-th robot mesh at the k-th ``rbt_idx`` entry."""
        hits = _entries(msg, self.blk_idx) if self.task_mesh_frame_handle is not None else []
        if hits:
            yield (self.task_mesh_frame_handle, *self._mesh_pose(msg, hits[-1], None))
        if self.mesh_frame_handles:
            for h, i in zip(self.mesh_frame_handles, _entries(msg, self.rbt_idx)):
                yield (h, *self._mesh_pose(msg, i, self.weld_translation))

    def _mesh_pose(self, msg, idx: int, weld):
        """``icp o SE3(q/|q|, (p + weld) s)`` of message entry ``idx`` as (wxyz, t), float64; ``weld`` None: the task mesh, not welded."""
        q = np.asarray(msg.quaternion[idx], dtype=np.float64)
        q = q / np.linalg.norm(q)
        R = self.Ri @ poses.quat_wxyz_to_matrix(q)
        p = np.asarray(msg.position[idx], dtype=np.float64)
        if weld is not None:
            p = p + weld
        return poses.matrix_to_quat_wxyz(R), self.Ri @ (p * self.scale_factor) + self.ti

    def _link_entries(self, msg) -> Tuple[List[int], int]:
        """``(idxs, k)``: the message entries of the robot's links, and how many of them drive link groups -- no more than there are
        forward-kinematics poses, link groups, or seven (:282)."""
        idxs = _entries(msg, self.rbt_idx)
        return idxs, min(len(idxs), len(self.fk), 7, len(self.splat_links_handler))

    def draw_handler(self, msg) -> None:
        """``msg``: lcmt_viewer_draw-shaped (num_links, robot_num[], position[][3], quaternion[][4] wxyz).  The
        k-th link of the robot (``robot_num == rbt_idx``, message order) drives splat group k, as in the reference
        (:227-314); all links are posed in one batch of small matrix products."""
        if self.task_mesh_frame_handle is not None or self.mesh_frame_handles:
            for h, wxyz, t in self._mesh_entries(msg):
                h.wxyz, h.position = wxyz, t
        idxs, k = self._link_entries(msg)
        for idx in idxs[len(self.fk):]:
            logging.warning(f"Warning: Received draw command for non-existent Link index {idx}.")
        if k == 0:
            return
        if self._fast and idxs[k - 1] == k - 1:          # the robot's links lead the message (Drake's order): no gather
            self.scene.set_link_poses(msg.quaternion[:k], msg.position[:k], owner=id(self))
            return
        q = np.asarray([msg.quaternion[i] for i in idxs[:k]], dtype=np.float64)
        p = np.asarray([msg.position[i] for i in idxs[:k]], dtype=np.float64)
        if self._fast:
            self.scene.set_link_poses(q, p, owner=id(self))      # float64 in C, the arithmetic below; handles read their rows back on demand
            return
        R, t = poses.link_splat_poses(self.scale_factor, self.Ri, self.ti, self._fkR[:k], self._fkt[:k], q, p, self.weld_translation)
        wxyz = poses.matrices_to_quats_wxyz(R)
        lock = getattr(self.scene, "lock", None)
        if lock is not None:
            lock.acquire()      # the k assignments are ONE update: a render on another thread sees all or none of it
        try:
            for j in range(k):
                h = self.splat_links_handler[j]
                h.wxyz = wxyz[j]
                h.position = t[j]
        finally:
            if lock is not None:
                lock.release()

    def link_pose_rows(self, msg) -> Tuple[np.ndarray, np.ndarray]:
        """The pose rows ``draw_handler(msg)`` would give this handler's link groups, WITHOUT touching the scene:
        ``(group indices [k], rows [k,12] float32)``.  Vectorised envs share one scene and keep a pose set per env
        (``SplatVecEnv``); the rows are the library's context-free ``sas_link_group_poses`` (float64 in C, the
        arithmetic of splat_handler.py:265-288), the same bits ``sas_set_link_poses`` writes."""
        from . import _capi
        idxs, k = self._link_entries(msg)
        groups = np.array([h.index for h in self.splat_links_handler[:k]], dtype=np.int64)
        rows = np.zeros((k, 12), np.float32)
        if k == 0:
            return groups, rows
        c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        q, p = c([msg.quaternion[i] for i in idxs[:k]]), c([msg.position[i] for i in idxs[:k]])
        Ri, ti, Rfk, tfk, weld = c(self.Ri), c(self.ti), c(self._fkR[:k]), c(self._fkt[:k]), c(self.weld_translation)
        rc = _capi.lib().sas_link_group_poses(k, float(self.scale_factor), Ri.ctypes.data, ti.ctypes.data, Rfk.ctypes.data, tfk.ctypes.data,
                                              weld.ctypes.data, q.ctypes.data, p.ctypes.data, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"sas_link_group_poses failed ({rc})")
        return groups, rows

    def get_attached_frame(self, body_name: str, local_frame_pos, msg) -> Tuple[np.ndarray, np.ndarray]:
        """``local_frame_pos``: the camera's ``local_frame`` (SE3-like, as the reference passes it, :316-319) or
        just its translation; only the translation is used -- added in world axes, the reference's behaviour."""
        if type(local_frame_pos) is poses.SE3:
            local_xyz = local_frame_pos.wxyz_xyz[4:]
        elif hasattr(local_frame_pos, "translation") or (isinstance(local_frame_pos, (tuple, list)) and len(local_frame_pos) == 2):
            local_xyz = poses.pose_wxyz_xyz(local_frame_pos)[1]
        else:
            local_xyz = np.asarray(local_frame_pos, dtype=np.float64).reshape(3)
        idx = msg.link_name.index("plant::" + body_name) if isinstance(msg.link_name, list) else list(msg.link_name).index("plant::" + body_name)
        if self._fast and hasattr(self.scene, "attached_frame"):
            return self.scene.attached_frame(msg.quaternion[idx], msg.position[idx], local_xyz, owner=id(self))
        R, t = poses.attached_frame(self.scale_factor, self.Ri, self.ti, msg.quaternion[idx], msg.position[idx], local_xyz)
        return poses.matrix_to_quat_wxyz(R), t

    def render(self, chs, cam_poses, render_size) -> List[np.ndarray]:
        """``render(chs, cam_poses: List[SE3], render_size)`` of the reference (:334-346): ``chs`` is the client
        handle (here the ``SplatScene``: ``get_render`` + a ``camera``), ``cam_poses`` SE3-like objects or
        ``(wxyz, xyz)`` pairs (None: the client's own camera), ``render_size[i] = [H, W]``.  Returns uint8
        [H,W,3] frames in camera order.  Cameras of equal size go to the GPU as one batch when the client
        offers ``get_renders`` (the reference renders them one by one)."""
        cam = _cameras(chs, cam_poses)
        n = len(cam)
        s0 = render_size[0] if n else None
        if n and hasattr(chs, "get_renders") and all(s[0] == s0[0] and s[1] == s0[1] for s in render_size[1:n]):
            return list(chs.get_renders(int(s0[0]), int(s0[1]), cam))      # the usual rig: every camera the same size, one batch
        out: List[Optional[np.ndarray]] = [None] * n
        for (H, W), idx in _by_size(render_size, n).items():
            if hasattr(chs, "get_renders"):
                imgs = chs.get_renders(H, W, [cam[i] for i in idx])
            else:
                imgs = [chs.get_render(height=H, width=W, wxyz=cam[i][0], position=cam[i][1]) for i in idx]
            for j, i in enumerate(idx):
                out[i] = np.asarray(imgs[j])
        return out

    def render_segmentation(self, chs, cam_poses, render_size) -> List[np.ndarray]:
        """``render`` for label images: one uint8 ``[H,W]`` per camera, the pose-row index of the splat group or mesh each
        pixel shows (``chs.row_names()`` names the rows; 255: nothing) -- ``SplatScene.get_segmentation``, one view at a time
        (feature frames are single views)."""
        return [chs.get_segmentation(int(s[0]), int(s[1]), wxyz=w, position=p)["labels"].cpu().numpy()
                for (w, p), s in zip(_cameras(chs, cam_poses), render_size)]

    def robot_frame(self) -> np.ndarray:
        """4x4 float64, splat scene -> the robot's metric frame: the inverse of the ICP similarity ``x_scene = s Ri x_robot + ti``
        (``poses.decompose_icp``), ``x_robot = Ri^T (x_scene - ti) / s``."""
        F = np.eye(4)
        F[:3, :3] = self.Ri.T / self.scale_factor
        F[:3, 3] = -(self.Ri.T @ self.ti) / self.scale_factor
        return F

    def render_point_cloud(self, chs, cam_poses, render_size, n_points: int, *, frame="scene", bounds=None, voxel_size: float = 0.0,
                           stride: int = 1, keep=None, **kw):
        """One fixed-size point cloud from all cameras of a step (``SplatScene.get_point_clouds``): ``n_points`` rows by
        farthest-point sampling over the cameras' depth pixels.  ``frame="scene"``: the splat's own frame; ``"robot"``: the
        robot's metric frame (``robot_frame()``: the inverse of the handler's ICP similarity) -- ``bounds`` and ``voxel_size`` are
        then metres of the simulator; a 4x4 array: that map from the scene.  The cameras must be one size (ValueError).  Returns
        the device tensors of ``get_point_clouds``."""
        cam = _cameras(chs, cam_poses)
        sizes = {(int(s[0]), int(s[1])) for s in render_size[:len(cam)]}
        if len(sizes) != 1:
            raise ValueError(f"render_point_cloud needs cameras of one size, got {sorted(sizes)}")
        if isinstance(frame, str):
            if frame not in ("scene", "robot"):
                raise ValueError(f"frame must be 'scene', 'robot' or a 4x4 matrix, got {frame!r}")
            frame = self.robot_frame() if frame == "robot" else None
        (H, W), = sizes
        return chs.get_point_clouds(H, W, cam, int(n_points), bounds=bounds, voxel_size=voxel_size, stride=stride, keep=keep, frame=frame, **kw)

    def reconstruct_mesh(self, rows, bounds, voxel_size: float, *, frame="robot", n_azimuth: int = 12, elevations=(20, 50, 80),
                         radius: Optional[float] = None, render_size=(240, 320), scene: Optional[SplatScene] = None, **fuse_kw) -> Dict[str, np.ndarray]:
        """A triangle mesh of what the rows ``rows`` (names or indices of ``scene.row_names()``; None: everything) show inside
        ``bounds`` ``(lo[3], hi[3])``: ``reconstruct.orbit_cameras`` around the bounds' centre, ``SplatScene.fuse_views`` into a
        volume of ``voxel_size`` cubes, ``surface_nets``.  ``frame`` as in ``render_point_cloud`` -- ``"robot"``: bounds, voxel size and
        the mesh are metres of the simulator; the orbit's up is that frame's +z.  ``radius`` (frame units; default: the bounds fit
        the view).  Returns ``{"vertices" [V,3] float64, "faces" [F,3] int32, "colors" [V,3] uint8}`` in that frame: ready for
        ``upload_meshes``, ``query_meshes`` or ``mesh_io.save_obj``."""
        from . import reconstruct
        chs = self.scene if scene is None else scene
        if isinstance(frame, str):
            if frame not in ("scene", "robot"):
                raise ValueError(f"frame must be 'scene', 'robot' or a 4x4 matrix, got {frame!r}")
            frame = self.robot_frame() if frame == "robot" else None
        F = np.eye(4) if frame is None else np.asarray(frame, np.float64).reshape(4, 4)
        b = np.asarray(bounds, np.float64).reshape(2, 3)
        vol = reconstruct.TsdfVolume(chs._raster, b[0], voxel_size, hi=b[1])
        H, W = int(render_size[0]), int(render_size[1])
        if radius is None:
            radius = reconstruct.orbit_radius(0.5 * float(np.linalg.norm(b[1] - b[0])), chs.camera.fov, H, W)
        # the orbit is laid out in the volume's frame and carried into the scene's: positions through inv(F), the cameras' axes
        # through its rotation (F is a similarity: a scaled rotation keeps the axes orthogonal)
        cams = reconstruct.orbit_cameras(0.5 * (b[0] + b[1]), radius, n_azimuth, elevations)
        if frame is not None:
            inv = np.linalg.inv(F)
            s = float(np.cbrt(abs(np.linalg.det(inv[:3, :3]))))
            cams = [(poses.matrix_to_quat_wxyz((inv[:3, :3] / s) @ poses.quat_wxyz_to_matrix(q)), inv[:3, :3] @ p + inv[:3, 3]) for q, p in cams]
        chs.fuse_views(vol, H, W, cams, keep=rows, frame=frame, **fuse_kw)
        v, f, c = vol.extract_mesh()
        return {"vertices": v, "faces": f, "colors": c}

    def point_cloud_obs(self, chs, cam_poses, render_size, n_points: int, **cfg) -> np.ndarray:
        """``render_point_cloud`` as an observation entry: float32 ``[n_points,6]``, xyz then rgb in 0..1; padding rows are zero."""
        o = self.render_point_cloud(chs, cam_poses, render_size, n_points, **cfg)
        out = np.zeros((int(n_points), 6), np.float32)
        out[:, :3] = o["points"][0].cpu().numpy()
        out[:, 3:] = o["colors"][0].cpu().numpy().astype(np.float32) / np.float32(255.0)
        return out

    OBS_MODES = ("rgb", "depth", "segmentation", "pointcloud")

    def render_observations(self, chs, cam_poses, render_size, modes=("rgb",)) -> List[Dict[str, np.ndarray]]:
        """``render`` for several modalities: one dict per camera with the ``modes`` asked for -- ``rgb`` uint8 ``[H,W,3]`` (the
        frame ``render`` returns), ``depth`` float32 ``[H,W]`` (the scene's depth with meshes as surfaces, 0 where nothing is
        seen) and ``segmentation`` uint8 ``[H,W]`` (``render_segmentation``'s labels).  Cameras of equal size are one call
        (``SplatScene.get_observations``: label frames); ``modes=("rgb",)`` alone goes through ``render``."""
        modes = _checked_modes(modes)
        if "pointcloud" in modes:
            raise ValueError("'pointcloud' is one cloud of all cameras, not a per-camera mode: render_point_cloud")
        if set(modes) <= {"rgb"}:
            return [{m: img for m in modes} for img in self.render(chs, cam_poses, render_size)]
        cam = _cameras(chs, cam_poses)
        want = tuple(k for k, m in (("rgb8", "rgb"), ("depth", "depth")) if m in modes)
        out: List[Dict[str, np.ndarray]] = [dict() for _ in cam]
        for (H, W), idx in _by_size(render_size, len(cam)).items():
            o = chs.get_observations(H, W, [cam[i] for i in idx], want=want + ("labels",))
            host = {k: v.cpu().numpy() for k, v in o.items()}
            for j, i in enumerate(idx):
                for m in modes:
                    out[i][m] = host["rgb8"][j] if m == "rgb" else host["depth"][j, :, :, 0] if m == "depth" else host["labels"][j]
        return out


class CameraRig:
    """Camera dictionary ``{id: {link_name, local_frame, type, render_size}}`` of the reference
    (examples/demo_pusht_splat.py:54-78; ``local_frame`` SE3-like or ``(wxyz, xyz)``), resolved to render
    poses.  Order: moving cameras, then viewport + static (splat_env_wrapper.py:33-55,146)."""

    def __init__(self, camera_setup_info: Dict):
        self.camera_setup_info = camera_setup_info
        self.moving = {k: v for k, v in camera_setup_info.items() if v.get("type") == "moving"}
        self.viewport = {k: v for k, v in camera_setup_info.items() if v.get("type") == "viewport"}
        fixed = {k: v for k, v in camera_setup_info.items() if v.get("type") in ("viewport", "static")}
        self.fixed_cam_poses = [poses.pose_wxyz_xyz(v["local_frame"]) for v in fixed.values()]
        self.render_cam_keys = list(self.moving.keys()) + list(fixed.keys())

    def poses(self, handler: SplatHandler, msg) -> List[Tuple[np.ndarray, np.ndarray]]:
        moving = [handler.get_attached_frame(v["link_name"], v["local_frame"], msg) for v in self.moving.values()]
        return moving + self.fixed_cam_poses

    def sizes(self) -> List[Sequence[int]]:
        return [self.camera_setup_info[k]["render_size"] for k in self.render_cam_keys]

    def get_obs(self, handler: SplatHandler, msg, obs_modes=("rgb",)) -> Dict[str, np.ndarray]:
        """``camera_i`` -> uint8 [3,H,W]  (splat_env_wrapper.py:132-138).  Uses the CURRENT message:
        the reference reads the one stored at reset (its moving cameras lag).  ``obs_modes`` beyond
        ``("rgb",)``: ``"depth"`` adds ``camera_i_depth`` float32 [1,H,W], ``"segmentation"`` ``camera_i_segmentation`` uint8
        [1,H,W] (``SplatHandler.render_observations``)."""
        cam_poses, sizes = self.poses(handler, msg), self.sizes()
        if tuple(obs_modes) == ("rgb",):
            imgs = handler.render(handler.scene, cam_poses, sizes)
            return {f"camera_{i}": np.moveaxis(img, -1, 0) for i, img in enumerate(imgs)}
        return camera_obs_dict(handler.render_observations(handler.scene, cam_poses, sizes, obs_modes), obs_modes)


def camera_obs_dict(per_camera: List[Dict[str, np.ndarray]], obs_modes) -> Dict[str, np.ndarray]:
    """The per-camera dicts of ``render_observations`` as observation entries, channels first: ``camera_i`` uint8 [3,H,W],
    ``camera_i_depth`` float32 [1,H,W], ``camera_i_segmentation`` uint8 [1,H,W], in the order of ``obs_modes``."""
    obs: Dict[str, np.ndarray] = {}
    for i, d in enumerate(per_camera):
        for m in obs_modes:
            obs[f"camera_{i}" if m == "rgb" else f"camera_{i}_{m}"] = np.moveaxis(d[m], -1, 0) if m == "rgb" else d[m][None]
    return obs
