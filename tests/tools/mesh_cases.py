"""Shared by the mesh tests (test_gpu_g_meshes.py, test_gpu_h_mesh_oracle.py, test_gpu_i_mesh_features.py, test_gpu_k_smooth_meshes.py
and their CPU files) and the fuzzer: meshes in camera space, the float64 ray cast, and the FIXED CASES that hold the HIP mesh frames
to oracle.mesh_ref + the depth-limited oracle.  Everything down to "GPU side" runs on the CPU; the GPU tests render the same inputs
and compare.  The scenes, cameras and frame helpers are scene_cases.py's, re-exported here.

A case is a dict: sc (scene arrays), cams [(V, K, W, H)], mesh (verts, tris, cols, groups, ka, kd, and normals / vcols [V,3] or None:
smooth shading, DESIGN.md 3 rule 2b), bg, poses (one [G,12] block per view, or None).  `expected(case, view)` gives the reference
frame, its `stable` mask and the counts the caps are taken from."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from scene_cases import GOLDEN, OUTS, config3_window, oracle_frame, ring, same, synthetic, to_numpy, twin, upload  # noqa: E402,F401
from oracle import mesh_ref  # noqa: E402
from sim_a_splat_amd.synthetic import make_scene  # noqa: E402

BG = (0.12, 0.34, 0.56)
MAX_EXCLUDED = 0.10      # `stable` may be false on at most this share of a frame (the coverage test's own allowance)
MIN_DRIVEN = 0.20        # share of a frame that is stable, mesh-covered, with list entries cut off AND entries kept
RGB_TOL = 1e-4           # the project's parity gate: float32 attribute planes against the float64 reference


# ---- meshes in camera space -------------------------------------------------------------------------------------------
def cam_to_world(cam, pc):
    V = np.asarray(cam[0], np.float64).reshape(4, 4)
    R, t = V[:3, :3], V[:3, 3]
    return (pc - t) @ R          # R^T (p - t)


def screen_quad(cam, d, u0, u1, v0, v1):
    """Two triangles at camera depth d whose corners project to (u, v) in [u0, u1] x [v0, v1]."""
    V, K, W, H = cam
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    uv = np.array([[u0, v0], [u1, v0], [u1, v1], [u0, v1]], np.float64)
    pc = np.stack([(uv[:, 0] - cx) * d / fx, (uv[:, 1] - cy) * d / fy, np.full(4, d)], 1)
    return cam_to_world(cam, pc).astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def full_quad(cam, d):
    W, H = cam[2], cam[3]
    return screen_quad(cam, d, -20.0, W + 20.0, -20.0, H + 20.0)


def tilted_quad(cam, z_a, z_b, u0=-20.0, u1=None, v0=-20.0, v1=None):
    """A plane rotated about both image axes, as two triangles with corners at (u0|u1, v0|v1) px: 1/z is linear in the pixel,
    z_a at the frame's corner (0, 0) and z_b at (W, H), 60 % of the sweep along x and 40 % along y.  World coordinates, float64."""
    V, K, W, H = cam
    u1 = W + 20.0 if u1 is None else u1
    v1 = H + 20.0 if v1 is None else v1
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    uv = np.array([[u0, v0], [u1, v0], [u1, v1], [u0, v1]], np.float64)
    w = 1.0 / z_a + (1.0 / z_b - 1.0 / z_a) * (0.6 * uv[:, 0] / W + 0.4 * uv[:, 1] / H)
    assert (w > 0).all()
    z = 1.0 / w
    pc = np.stack([(uv[:, 0] - cx) * z / fx, (uv[:, 1] - cy) * z / fy, z], 1)
    return cam_to_world(cam, pc), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def to_group_local(world, Rt_row):
    """pose^-1 of world points: the mesh-local vertices that the group's pose carries to `world`."""
    Rt = np.asarray(Rt_row, np.float64).reshape(3, 4)
    return ((np.asarray(world, np.float64) - Rt[:, 3]) @ Rt[:, :3]).astype(np.float32)


def ray_cast(cam, verts, tris, eps=(0.0, 0.0), camera_frame=False, want_depth=False):
    """Index of the nearest triangle hit by the ray through every pixel centre (+ eps offsets), -1 for none; float64
    Moeller-Trumbore.  A hit counts when its camera depth is >= 0.01 (the near plane).  camera_frame: verts are camera-frame
    points already ([T,3,3] with tris None, or [V,3])."""
    V, K, W, H = cam
    if camera_frame:
        pc = np.asarray(verts, np.float64).reshape(-1, 3)
        if tris is None:
            tris = np.arange(pc.shape[0]).reshape(-1, 3)
    else:
        Vd = np.asarray(V, np.float64).reshape(4, 4)
        pc = np.asarray(verts, np.float64) @ Vd[:3, :3].T + Vd[:3, 3]
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    ys, xs = np.mgrid[0:H, 0:W]
    dx = ((xs + 0.5 + eps[0]) - cx) / fx
    dy = ((ys + 0.5 + eps[1]) - cy) / fy
    D = np.stack([dx, dy, np.ones_like(dx)], -1).reshape(-1, 3)
    best = np.full(D.shape[0], np.inf)
    idx = np.full(D.shape[0], -1)
    for k, (a, b, c) in enumerate(tris):
        A, B, Cc = pc[a], pc[b], pc[c]
        if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(Cc).all()):
            continue
        e1, e2 = B - A, Cc - A
        pv = np.cross(D, e2)
        det = pv @ e1
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = 1.0 / det
            u = (pv @ -A) * inv
            qv = np.cross(-A, e1)
            v = (D @ qv) * inv
            s = (e2 @ qv) * inv            # ray parameter = camera depth (D.z == 1)
            hit = (np.abs(det) > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (s >= 0.01) & (s < best)
        best[hit] = s[hit]
        idx[hit] = k
    if want_depth:
        return idx.reshape(H, W), best.reshape(H, W)
    return idx.reshape(H, W)


def stable_ref(cam, verts, tris, tol=1e-3):
    maps = [ray_cast(cam, verts, tris, e) for e in ((0, 0), (tol, 0), (-tol, 0), (0, tol), (0, -tol))]
    stable = np.all([m == maps[0] for m in maps[1:]], axis=0)
    return maps[0], stable


def colours(n, seed):
    rng = np.random.default_rng(seed)
    cols = set()
    while len(cols) < n:
        cols.add(tuple(int(x) for x in rng.integers(10, 246, 3)))
    cols = np.array(sorted(cols), np.float64)
    rng.shuffle(cols)
    return cols


def random_triangles(cam, n, seed):
    """Triangles in camera space: some cross the near plane, some reach beyond the frame, many overlap; then to world."""
    rng = np.random.default_rng(seed)
    V, K, W, H = cam
    fx, cx, fy, cy = float(K[0, 0]), float(K[0, 2]), float(K[1, 1]), float(K[1, 2])
    pts = []
    for k in range(n):
        zc = rng.uniform(0.5, 6.0)
        u = rng.uniform(-0.3 * W, 1.3 * W, 3)
        v = rng.uniform(-0.3 * H, 1.3 * H, 3)
        z = zc + rng.uniform(-0.4, 0.4, 3)
        if k % 7 == 0:
            z[0] = -0.5                                   # crosses the near plane
        pts.append(np.stack([(u - cx) * np.abs(z) / fx, (v - cy) * np.abs(z) / fy, z], 1))
    pc = np.concatenate(pts)
    tris = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    # two triangles sharing an edge (a split quad), flat in depth
    q, qt = screen_quad(cam, 2.0, 0.3 * W, 0.7 * W, 0.2 * H, 0.8 * H)
    verts = np.concatenate([cam_to_world(cam, pc), q.astype(np.float64)]).astype(np.float32)
    tris = np.concatenate([tris, qt + 3 * n]).astype(np.int32)
    return verts, tris


def subdivide(verts, tris, levels):
    """Every triangle into four, `levels` times (midpoints are not shared: the kernels take any triangle soup)."""
    tri = np.asarray(verts, np.float64)[np.asarray(tris)]          # [T,3,3]
    for _ in range(levels):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)
        tri = np.concatenate([np.stack(t, 1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    return tri.reshape(-1, 3), np.arange(3 * tri.shape[0], dtype=np.int32).reshape(-1, 3)


# ---- expectation ------------------------------------------------------------------------------------------------------
def visible_depths(sc, cam, Rt=None):
    d = oracle_frame(sc, cam, BG, Rt=Rt, dump=True)
    vis = (d["radii"][:, 0] > 0) & (d["radii"][:, 1] > 0)
    return np.sort(d["depths"][vis].astype(np.float64))


def view_poses(case, view=0):
    """The pose rows view `view` of a case is rendered with (None: a scene without groups)."""
    sc = case["sc"]
    if sc["gid"] is None:
        return None
    Rt = None if case.get("poses") is None else case["poses"][view]
    return np.asarray(sc["Rt"] if Rt is None else Rt, np.float32).reshape(-1, 12)


def expected(case, view=0, depth_mode=0, want_frame=True, attributes=True):
    """The reference of one view of a case: frame (the depth-limited oracle's outputs; want_frame), ref (oracle.mesh_ref.reference;
    attributes=False: the mesh drawn flat, whatever normals it carries), stable / cut / length per pixel, and the counts the caps are
    asserted on.  One dump render, one reference, one frame render."""
    sc, cam, m = case["sc"], case["cams"][view], case["mesh"]
    V, K, W, H = cam
    Rt = view_poses(case, view)
    dump = oracle_frame(sc, cam, case["bg"], Rt=Rt, dump=True)
    attr = dict(vertex_normals=m["normals"], vertex_colors=m["vcols"]) if attributes else {}
    ref = mesh_ref.reference(m["verts"], m["tris"], m["cols"], m["groups"], Rt, m["ka"], m["kd"], V, K, W, H, **attr)
    st = mesh_ref.stability(ref, dump)
    zlim, bgmap = mesh_ref.frame_inputs(ref, case["bg"])
    frame = oracle_frame(sc, cam, case["bg"], Rt=Rt, zlim=zlim, bgmap=bgmap, depth_mode=depth_mode) if want_frame else None
    stable, cut, length = st["stable"], st["cut"], st["length"]
    covered = ref["winner"] >= 0
    driven = stable & covered & (cut > 0) & (cut < length)
    # the 256-entry batches of the tile loop: a compared tile longer than 512 entries whose stable pixels stop both inside
    # the first batch and after it
    both = 0
    tw, th = (W + 15) // 16, (H + 15) // 16
    for t in range(tw * th):
        sl = (slice(16 * (t // tw), 16 * (t // tw) + 16), slice(16 * (t % tw), 16 * (t % tw) + 16))
        if length[sl].max() > 512:
            s_, c_, l_ = stable[sl] & covered[sl], cut[sl], length[sl]
            both += bool((s_ & (c_ < 256)).any() and (s_ & (c_ >= 256) & (c_ < l_)).any())
    return dict(frame=frame, ref=ref, stable=stable, cut=cut, length=length, zlim=zlim, excluded=float(1.0 - stable.mean()),
                driven=float(driven.mean()), covered=float(covered.mean()), tiles_cut_in_both_batches=int(both),
                longest_list=int(length[stable].max()) if stable.any() else 0, n_cut=int((covered & (cut < length)).sum()))


def report(name, case, e):
    W, H = case["cams"][0][2], case["cams"][0][3]
    return (f"{name}: {W}x{H} triangles={len(case['mesh']['tris'])} compared={int(e['stable'].sum())} excluded={int((~e['stable']).sum())} "
            f"({100 * e['excluded']:.2f} %) cut={e['n_cut']} driven={100 * e['driven']:.1f} % longest_list={e['longest_list']} "
            f"tiles_cut_in_both_batches={e['tiles_cut_in_both_batches']}")


# ---- the fixed cases --------------------------------------------------------------------------------------------------
C_PLANE = (0.9, 0.2, 0.1)


def _mesh(verts, tris, cols, groups=None, ka=0.4, kd=0.6, normals=None, vcols=None):
    f32 = lambda a: None if a is None else np.asarray(a, np.float32)
    return dict(verts=f32(verts), tris=np.asarray(tris, np.int32), cols=f32(cols), groups=None if groups is None else np.asarray(groups, np.uint8),
                ka=float(ka), kd=float(kd), normals=f32(normals), vcols=f32(vcols))


def _plane_case(sc, cam, group=None, edges_inside=False):
    """A tilted plane through the cloud: z_m sweeps from the 10 % to the 90 % quantile of the visible depths across the frame."""
    z = visible_depths(sc, cam)
    za, zb = float(np.quantile(z, 0.10)), float(np.quantile(z, 0.90))
    W, H = cam[2], cam[3]
    kw = {}
    if edges_inside:      # the quad's right and lower edges run inside the ragged last tiles
        kw = dict(u1=16 * (W // 16) + 0.83 * (W % 16), v1=16 * (H // 16) + 0.83 * (H % 16))
    world, tris = tilted_quad(cam, za, zb, **kw)
    if sc["gid"] is not None:
        g = 1 if group is None else group
        verts, groups = to_group_local(world, sc["Rt"].reshape(-1, 12)[g]), [g, g]
    else:
        verts, groups = world.astype(np.float32), None
    cols = np.array([C_PLANE, (0.2, 0.8, 0.3)], np.float32)
    return dict(sc=sc, cams=[cam], mesh=_mesh(verts, tris, cols, groups), bg=BG, poses=None)


def case_plane(name):
    sc, cam = config3_window() if name == "cfg3" else twin(name)
    return _plane_case(sc, cam)


PLANE_SCENES = ("n2k_groups", "doorb", "dense", "inside", "cfg3")


def tblock(scale):
    from sim_a_splat_amd.mesh_io import load_obj
    v, f = load_obj(GOLDEN / "tblock_paper.obj")
    return (v * scale).astype(np.float32), f.astype(np.int32)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose_rows(sc, group, ang, t):
    """The scene's pose rows with `group` rotated by the angles `ang` and moved to `t`."""
    Rt = sc["Rt"].reshape(-1, 12).astype(np.float32).copy()
    Rt[group] = np.concatenate([_rot(*ang), np.asarray(t, np.float64)[:, None]], 1).reshape(12)
    return Rt


TBLOCK_POSES = (((0.9, 0.3, 0.4), (0.0, 0.55, 0.0)), ((-0.6, 0.8, -0.2), (0.15, 0.45, 0.1)))


def case_tblock():
    """The T-block on pose group 2 of a grouped scene, inside the cloud; two views of one camera, each with its own pose set."""
    sc = synthetic(6000, 31, 0.03, n_groups=3)
    cam = ring(320, 240, 560.0, yaw=20.0)
    v, f = tblock(6.0)
    from sim_a_splat_amd.handler import TASK_MESH_COLOR
    return dict(sc=sc, cams=[cam, cam], mesh=_mesh(v, f, TASK_MESH_COLOR, np.full(len(f), 2)), bg=BG,
                poses=[pose_rows(sc, 2, ang, t) for ang, t in TBLOCK_POSES])


def case_soup():
    sc, cam = twin("n2k")
    verts, tris = random_triangles(cam, 30, 7)
    return dict(sc=sc, cams=[cam], mesh=_mesh(verts, tris, colours(len(tris), 3) / 255.0), bg=BG, poses=None)


def case_size(W, H):
    sc = synthetic(4000 if W > 100 else 1500, 41 + W, 0.05)
    return _plane_case(sc, ring(W, H, 0.9 * max(W, H), yaw=35.0), edges_inside=True)


def case_1080p():
    """1920x1080 over about 20 k Gaussians, two intersecting T-blocks subdivided to 3 584 small triangles: 8 160 tiles."""
    sc = synthetic(20000, 51, 0.04, n_groups=2)
    cam = ring(1920, 1080, 1400.0, yaw=10.0)
    v, f = tblock(9.0)
    vs, fs, gs = [], [], []
    for k, (ang, t) in enumerate((((0.8, 0.2, 0.3), (-0.2, 0.8, 0.0)), ((-0.5, 0.9, 0.1), (0.3, 0.6, 0.1)))):
        w = v.astype(np.float64) @ _rot(*ang).T + np.asarray(t)
        sv, sf = subdivide(w, f, 3)
        vs.append(to_group_local(sv, sc["Rt"].reshape(-1, 12)[k]))
        fs.append(sf + sum(len(x) for x in vs[:-1]))
        gs.append(np.full(len(sf), k))
    tris = np.concatenate(fs)
    return dict(sc=sc, cams=[cam], mesh=_mesh(np.concatenate(vs), tris, colours(len(tris), 5) / 255.0, np.concatenate(gs)), bg=BG,
                poses=None)


def case_entry_points():
    """The tilted plane of n2k_groups seen by two different cameras, each view with a pose set of its own."""
    sc, cam = twin("n2k_groups")
    base = _plane_case(sc, cam)
    V, K, W, H = cam
    V2 = V.copy()
    V2[:3, 3] += np.array([0.12, -0.07, 0.2], np.float32)
    K2 = K.copy()
    K2[0, 0] *= 1.1
    K2[1, 2] += 3.0
    R2 = sc["Rt"].reshape(-1, 12).astype(np.float32).copy()
    R2[:, 3] += 0.05
    R2[1, 11] += 0.08
    base["cams"] = [cam, (V2, K2, W, H)]
    base["poses"] = [sc["Rt"].reshape(-1, 12).astype(np.float32), R2]
    return base


FIXED_CASES = {**{f"plane_{n}": (lambda n=n: case_plane(n)) for n in PLANE_SCENES},
               "tblock": case_tblock, "soup": case_soup, "size_250x187": lambda: case_size(250, 187),
               "size_17x33": lambda: case_size(17, 33), "full_hd": case_1080p, "entry_points": case_entry_points}
COVERAGE_IS_DRAWN = ("soup",)      # the driven-share cap does not apply: coverage is whatever was drawn


# ---- the T-block through SplatHandler(meshes=("task",)) -----------------------------------------------------------------
class DrawMsg:
    def __init__(self, robot_num, quaternion, position):
        self.num_links = len(robot_num)
        self.robot_num, self.quaternion, self.position = robot_num, [np.asarray(q) for q in quaternion], [np.asarray(p) for p in position]


def handler_setup():
    """What SplatHandler.from_arrays takes (two link groups + the static rest), a draw message that puts the task block
    inside the cloud, and a camera 0.75 units in front of it."""
    import torch
    from sim_a_splat_amd import poses
    from sim_a_splat_amd.covariance import compute_cov, sh2rgb
    sc = make_scene(4000, seed=2, log_scale_mean=float(np.log(0.03)))
    covs = compute_cov(torch.from_numpy(sc.quats), torch.from_numpy(sc.scales)).numpy()
    cols = np.clip(sh2rgb(torch.from_numpy(sc.sh[:, 0])).numpy(), 0, 1)
    masks = {"link0": np.arange(4000) < 500, "link1": (np.arange(4000) >= 500) & (np.arange(4000) < 900)}
    ang = 0.4
    icp = np.eye(4)
    icp[:3, :3] = 5.0 * np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    icp[:3, 3] = (0.2, -0.1, 0.05)
    fk = [np.eye(4), np.eye(4)]
    s, Ri, ti = poses.decompose_icp(icp)
    t_world = np.array([0.1, 0.3, 0.0])
    p = Ri.T @ (t_world - ti) / s
    q = np.array([0.9, 0.2, -0.3, 0.25]) * 2.0
    msg = DrawMsg([3, 3, 2], [(1, 0, 0, 0), (1, 0, 0, 0), q], [(0, 0, 0), (0.01, 0, 0), p])
    cam = (np.array([1.0, 0.0, 0.0, 0.0]), t_world + np.array([0.05, -0.3, -0.75]))
    return dict(args=(sc.means, covs, cols, sc.opacities, masks, icp, fk), msg=msg, cam=cam, size=(240, 320), scene=sc, covs=covs, cols=cols,
                masks=masks, icp=icp, fk=fk)


def handler_predicted_rows(hs, robot=False):
    """The pose rows draw_handler gives the groups (links, the static rest, the task mesh), restated on the CPU.  robot: and the rows
    of the two robot meshes.  The k-th message link poses its mesh with icp o SE3(q / |q|, (p + weld) s) (the weld is zero here),
    through the handle's quaternion."""
    from sim_a_splat_amd import poses
    s, Ri, ti = poses.decompose_icp(hs["icp"])
    msg = hs["msg"]

    def mesh_row(k):
        q = np.asarray(msg.quaternion[k], np.float64)
        R = Ri @ poses.quat_wxyz_to_matrix(q / np.linalg.norm(q))
        t = Ri @ (np.asarray(msg.position[k], np.float64) * s) + ti
        return poses.rt_to_row12(poses.quat_wxyz_to_matrix(poses.matrix_to_quat_wxyz(R)), t)

    q = np.asarray(msg.quaternion[:2], np.float64)
    p = np.asarray(msg.position[:2], np.float64)
    R, t = poses.link_splat_poses(s, Ri, ti, np.stack([T[:3, :3] for T in hs["fk"]]), np.stack([T[:3, 3] for T in hs["fk"]]), q, p,
                                  np.zeros(3))
    rows = [poses.rt_to_row12(poses.quat_wxyz_to_matrix(poses.matrix_to_quat_wxyz(R[k])), t[k]) for k in range(2)]
    rows += [poses.rt_to_row12(np.eye(3), np.zeros(3)), mesh_row(2)] + ([mesh_row(0), mesh_row(1)] if robot else [])
    return np.stack(rows).astype(np.float32).reshape(-1, 12)


def case_handler(hs, rows, V, K, robot=False):
    """The handler's frame as a case: the Gaussians in registration order (links, then the rest), the block, flat, on row 3.  robot:
    mesh_smooth_cases.robot_links, smooth, on rows 4 and 5 (zero normals for the block's vertices)."""
    from sim_a_splat_amd import mesh_io, poses
    from sim_a_splat_amd.handler import TASK_MESH_COLOR
    sc, masks, covs = hs["scene"], hs["masks"], hs["covs"]
    idx = [np.nonzero(masks[f"link{i}"])[0] for i in range(2)]
    rest = np.nonzero(~np.logical_or.reduce(list(masks.values())))[0]
    order = np.concatenate(idx + [rest])
    gid = np.concatenate([np.full(len(ix), i, np.uint8) for i, ix in enumerate(idx)] + [np.full(len(rest), 2, np.uint8)])
    cov6 = np.stack([covs[:, 0, 0], covs[:, 0, 1], covs[:, 0, 2], covs[:, 1, 1], covs[:, 1, 2], covs[:, 2, 2]], 1)[order]
    G = 6 if robot else 4
    scd = dict(means=sc.means[order], op=sc.opacities[order], colors=hs["cols"][order], sh=-1, quats=None, scales=None, cov6=cov6, gid=gid,
               G=G, Rt=np.asarray(rows, np.float32).reshape(G, 12))
    s = float(poses.decompose_icp(hs["icp"])[0])
    v, f = mesh_io.load_obj(GOLDEN / "tblock_paper.obj")
    verts, tris, groups = [(np.asarray(v, np.float64) * s).astype(np.float32)], [np.asarray(f, np.int32)], [np.full(len(f), 3)]
    cols, normals = TASK_MESH_COLOR, None
    if robot:
        from mesh_smooth_cases import robot_links
        cols, normals = [np.tile(np.asarray(TASK_MESH_COLOR, np.float32), (len(f), 1))], [np.zeros_like(verts[0])]
        for k, (lv, lf, rgb) in enumerate(robot_links()):
            lv, lf = mesh_io.weld(lv, lf)
            tris.append(lf + sum(len(x) for x in verts))
            verts.append((lv * s).astype(np.float32))
            cols.append(np.tile(np.asarray(rgb, np.float32), (len(lf), 1)))
            groups.append(np.full(len(lf), 4 + k))
            normals.append(mesh_io.vertex_normals(lv, lf))
        cols, normals = np.concatenate(cols), np.concatenate(normals)
    H, W = hs["size"]
    return dict(sc=scd, cams=[(np.asarray(V, np.float32), np.asarray(K, np.float32), W, H)],
                mesh=_mesh(np.concatenate(verts), np.concatenate(tris), cols, np.concatenate(groups), normals=normals), bg=(0.0, 0.0, 0.0), poses=None)


def case_handler_cpu(robot=False):
    from sim_a_splat_amd.scene import DEFAULT_VERTICAL_FOV, SplatScene
    hs = handler_setup()
    H, W = hs["size"]
    V, K = SplatScene._view_and_K(H, W, hs["cam"][0], hs["cam"][1], DEFAULT_VERTICAL_FOV)
    return case_handler(hs, handler_predicted_rows(hs, robot), V, K, robot)


FIXED_CASES["handler"] = case_handler_cpu


# ---- GPU side: what the tests do with a Rasterizer and an expectation -------------------------------------------------------
def upload_case(r, case, attributes=True):
    m = case["mesh"]
    upload(r, case["sc"])
    kw = dict(vertex_normals=m["normals"], vertex_colors=m["vcols"]) if attributes and m["normals"] is not None else {}
    r.upload_meshes(m["verts"], m["tris"], m["cols"], groups=m["groups"], ambient=m["ka"], diffuse=m["kd"], **kw)


def single(r, case, view=0, **kw):
    V, K, W, H = case["cams"][view]
    return to_numpy(r.render(V, K, W, H, case["bg"], want=OUTS, **kw))


def expect(name, case, view=0):
    """expected(case, view), printed and held to the caps."""
    e = expected(case, view)
    print(report(f"{name}[{view}]", case, e))
    assert e["excluded"] <= MAX_EXCLUDED, report(name, case, e)
    if name not in COVERAGE_IS_DRAWN:
        assert e["driven"] >= MIN_DRIVEN, report(name, case, e)
    return e


def compare_stable(got, frame, stable, fill=False, bits=True):
    """Differences between a GPU frame and the reference frame (rendered with depth_mode 0) on the stable pixels.  fill: the GPU
    frame has the depth fill (alpha == 0 -> the frame's largest expected depth).  The frame's maximum runs over ALL pixels, and an
    unstable pixel may legitimately hold another depth on the GPU than in the reference; so the filled value is held to the
    larger of the reference's maximum over the stable pixels and the GPU's own depths on the unstable ones -- the reference's
    own maximum whenever that is attained on a stable pixel and no unstable GPU pixel lies above it."""
    diffs = []
    for k, g in got.items():
        want, mask = np.asarray(frame[k]), stable
        if k == "depth" and fill:
            ed, a = want[..., 0], np.asarray(frame["alpha"])[..., 0]
            loose = ~stable & (np.asarray(got["alpha"])[..., 0] > 0)
            m = max(ed[stable].max(initial=0.0), np.asarray(g)[..., 0][loose].max(initial=0.0))
            want = np.where(a > 0, ed, np.float32(m))[..., None].astype(np.float32)
        x, y = np.asarray(g)[mask], want[mask]
        eq = np.array_equal(x.view(np.uint8), y.view(np.uint8)) if bits else np.array_equal(x, y, equal_nan=x.dtype != np.uint8)
        if not eq:
            d = np.abs(x.astype(np.float64) - y.astype(np.float64))
            diffs.append(f"{k}: {int((d > 0).sum())} values differ on stable pixels, max {np.nanmax(d):.3e}")
    return diffs


def compare(got, e, fill=False, bits=True):
    """A GPU frame against the expectation `e`, on the reference's stable pixels: alpha and depth bit-equal; rgb and rgb8 bit-equal
    where the winner is a flat triangle or none, and where it is smooth rgb within RGB_TOL, rgb8 within 1 LSB (the kernel interpolates
    float32 attribute planes, the reference float64 barycentrics).  Returns (problems, max |rgb| error, max rgb8 error) -- the figures
    over the stable smooth pixels.  A frame without smooth pixels: compare_stable on every output."""
    frame, stable, sp = e["frame"], e["stable"], e["ref"]["smooth_pixel"]
    pick = lambda *keys: {k: v for k, v in got.items() if k in keys}
    probs = compare_stable(pick("alpha", "depth"), frame, stable, fill, bits) + compare_stable(pick("rgb", "rgb8"), frame, stable & ~sp, fill, bits)
    on = stable & sp
    err = err8 = 0.0
    if "rgb" in got and on.any():
        err = float(np.abs(np.asarray(got["rgb"], np.float64)[on] - np.asarray(frame["rgb"], np.float64)[on]).max())
        if not err <= RGB_TOL:
            probs.append(f"rgb: max {err:.3e} on stable smooth pixels > {RGB_TOL}")
    if "rgb8" in got and on.any():
        err8 = float(np.abs(np.asarray(got["rgb8"]).astype(np.int64)[on] - np.asarray(frame["rgb8"]).astype(np.int64)[on]).max())
        if err8 > 1:
            probs.append(f"rgb8: max {err8:.0f} LSB on stable smooth pixels")
    return probs, err, err8
