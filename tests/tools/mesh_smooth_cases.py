"""The fixed cases of smooth-shaded meshes (DESIGN.md 3 "Meshes", rule 2b): mesh_cases' case dicts whose ``mesh`` carries ``normals [V,3]``
and, optionally, ``vcols [V,3]``.  mesh_cases.expected / upload_case / compare take them as they take the flat ones.  CPU only."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_cases as mc  # noqa: E402

RGB_TOL, pose_rows = mc.RGB_TOL, mc.pose_rows
SPHERE_POSE = ((0.9, 0.3, 0.4), (0.0, 0.1, 0.0))


def uv_sphere(r, nu, nv):
    """A UV sphere about the origin: nu segments around, nv from pole to pole; 2 nu (nv - 1) triangles on 2 + nu (nv - 1) shared
    vertices, and the unit radial normals."""
    th = np.pi * np.arange(1, nv) / nv
    ph = 2.0 * np.pi * np.arange(nu) / nu
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nu))], -1)
    n = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    at = lambda i, j: 1 + i * nu + (j % nu)
    south = 1 + nu * (nv - 1)
    tris = [[0, at(0, j), at(0, j + 1)] for j in range(nu)]
    for i in range(nv - 2):
        for j in range(nu):
            tris += [[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]]
    tris += [[south, at(nv - 2, j + 1), at(nv - 2, j)] for j in range(nu)]
    return (r * n).astype(np.float32), np.asarray(tris, np.int32), n.astype(np.float32)


def sphere_parts(r, nu, nv, seed=5):
    v, f, n = uv_sphere(r, nu, nv)
    vc = np.random.default_rng(seed).uniform(0.15, 1.0, size=v.shape).astype(np.float32)
    return v, f, n, vc


def case_sphere(W, H, f, n, ls, r, nu, nv):
    sc = mc.synthetic(n, 31, ls, n_groups=3)
    cam = mc.ring(W, H, f, yaw=20.0)
    v, t, nr, vc = sphere_parts(r, nu, nv)
    mesh = mc._mesh(v, t, (0.7, 0.7, 0.7), np.full(len(t), 2), normals=nr, vcols=vc)
    return dict(sc=sc, cams=[cam], mesh=mesh, bg=mc.BG, poses=[pose_rows(sc, 2, *SPHERE_POSE)])


SPHERES = {"sphere_qvga": (320, 240, 560.0, 6000, 0.03, 0.7, 48, 24), "sphere_small": (96, 64, 90.0, 1500, 0.05, 0.8, 16, 8),
           "sphere_ragged": (33, 17, 30.0, 1500, 0.05, 0.8, 12, 6), "sphere_dense": (96, 64, 90.0, 1500, 0.05, 0.8, 128, 64)}


def case_mixed():
    """The T-block, flat, on group 1 and the sphere_small sphere, smooth, on group 2 in ONE upload (zero normals for the block's
    vertices); two views of one camera, each with its own pose set."""
    W, H, f, n, ls, r, nu, nv = SPHERES["sphere_small"]
    sc = mc.synthetic(n, 31, ls, n_groups=3)
    cam = mc.ring(W, H, f, yaw=20.0)
    bv, bf = mc.tblock(6.0)
    sv, sf, sn, svc = sphere_parts(r, nu, nv)
    from sim_a_splat_amd.handler import TASK_MESH_COLOR
    verts = np.concatenate([bv, sv])
    tris = np.concatenate([bf, sf + len(bv)])
    cols = np.concatenate([np.tile(np.asarray(TASK_MESH_COLOR, np.float32), (len(bf), 1)), np.full((len(sf), 3), 0.7, np.float32)])
    groups = np.concatenate([np.full(len(bf), 1), np.full(len(sf), 2)])
    normals = np.concatenate([np.zeros_like(bv), sn])
    vcols = np.concatenate([np.full(bv.shape, 0.25, np.float32), svc])      # (the block's are never read: its triangles are flat)
    poses = []
    for (bang, bt), (sang, st) in zip((((0.9, 0.3, 0.4), (-0.75, 0.1, 0.2)), ((-0.6, 0.8, -0.2), (-0.6, 0.0, 0.4))),
                                      (((0.9, 0.3, 0.4), (0.55, 0.1, 0.0)), ((0.2, -0.5, 1.1), (0.6, -0.05, 0.3)))):
        Rt = pose_rows(sc, 1, bang, bt)
        Rt[2] = np.concatenate([mc._rot(*sang), np.asarray(st, np.float64)[:, None]], 1).reshape(12)
        poses.append(Rt)
    return dict(sc=sc, cams=[cam, cam], mesh=mc._mesh(verts, tris, cols, groups, normals=normals, vcols=vcols), bg=mc.BG, poses=poses)


NEAR_A = np.array([[0.03125, -0.03125, 0.015625], [-0.03125, 0.046875, 0.03125], [0.015625, 0.03125, -0.046875]])   # colour channel x world axis
NEAR_B = np.array([0.5, 0.5, 0.5])


def near_clip_field(X):
    """The affine colour field of case_near_clip at world points ``X [...,3]``."""
    return np.asarray(X, np.float64) @ NEAR_A.T + NEAR_B


def case_near_clip():
    """A tilted smooth quad through the cloud whose first corner lies BEHIND the near plane: both of its triangles are clipped, one
    into two records.  ka = 1, kd = 0 and vertex colours that are an affine function of the world position: the frame must show that
    field at every hit point, whatever the clip did."""
    W, H, f, n, ls = 96, 64, 90.0, 1500, 0.05
    sc = mc.synthetic(n, 31, ls, n_groups=3)
    cam = mc.ring(W, H, f, yaw=20.0)
    # the plane z = 2.6 + 1.2 x + 0.5 y of the camera frame: it leaves the frame's left edge at z = 1.6, in front of the cloud, and its
    # right edge at z = 7, behind it; the corner (-3, -3) has z = -2.5
    xy = np.array([[-3.0, -3.0], [5.0, -3.0], [5.0, 3.0], [-3.0, 3.0]])
    pc = np.concatenate([xy, (2.6 + 1.2 * xy[:, :1] + 0.5 * xy[:, 1:])], 1)
    assert (pc[:, 2] < 0.01).sum() == 1
    world, tris = mc.cam_to_world(cam, pc), np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    verts = world.astype(np.float32)                                     # group 0: the identity pose
    vcols = near_clip_field(verts.astype(np.float64))
    assert vcols.min() >= 0.0 and vcols.max() <= 1.0, (vcols.min(), vcols.max(), verts)
    normals = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (4, 1))
    mesh = mc._mesh(verts, tris, (0.5, 0.5, 0.5), np.zeros(len(tris)), ka=1.0, kd=0.0, normals=normals, vcols=vcols)
    return dict(sc=sc, cams=[cam], mesh=mesh, bg=mc.BG, poses=None)


def case_xarm6_base():
    """One real link, as a loader and welding check on genuine data: the xarm6 base visual (an STL: three private vertices per
    facet), welded, with computed vertex normals, 8 x on group 2 inside the cloud; no vertex colours."""
    from sim_a_splat_amd import mesh_io
    v, f = mesh_io.load_mesh(mc.GOLDEN / "xarm6_base.stl")
    T = len(f)
    v, f = mesh_io.weld(v, f)
    assert len(f) == T and len(v) < 3 * T
    n = mesh_io.vertex_normals(v, f)
    sc = mc.synthetic(1500, 31, 0.05, n_groups=3)
    cam = mc.ring(96, 64, 90.0, yaw=20.0)
    mesh = mc._mesh((v - v.mean(0)) * 8.0, f, (0.75, 0.75, 0.8), np.full(T, 2), normals=n)
    return dict(sc=sc, cams=[cam], mesh=mesh, bg=mc.BG, poses=[pose_rows(sc, 2, (1.2, 0.3, 0.4), (0.0, 0.1, 0.2))])


# ---- the handler with meshes=("task", "robot") over procedural links ------------------------------------------------------------
def robot_links():
    """Two procedural links as SplatHandler takes them from arrays: (vertices, faces, rgb), each face with three private vertices as
    an STL has them (the handler welds); offset towards the camera of mesh_cases.handler_setup, in front of most of the cloud."""
    out = []
    for r, nu, nv, off, rgb in ((0.03, 12, 6, (0.0, 0.0, -0.09), (0.2, 0.5, 0.9)), (0.022, 10, 5, (0.05, 0.03, -0.1), (0.9, 0.8, 0.2))):
        v, f, _ = uv_sphere(r, nu, nv)
        v = v.astype(np.float64) * np.array([1.0, 1.6, 1.0]) + np.asarray(off)
        out.append((v[f.reshape(-1)], np.arange(3 * len(f)).reshape(-1, 3), rgb))
    return out


FIXED_CASES = {**{k: (lambda a=a: case_sphere(*a)) for k, a in SPHERES.items()}, "mixed": case_mixed, "near_clip": case_near_clip,
               "entry_points": lambda: case_sphere(*SPHERES["sphere_small"]), "xarm6_base": case_xarm6_base, "handler": lambda: mc.case_handler_cpu(robot=True)}
