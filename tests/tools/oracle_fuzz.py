"""Differential fuzzer: the HIP path (through the C ABI) against the C oracle on randomly drawn scenes, cameras and entry points.
Every output -- rgb, accumulation, expected depth, uint8 frame, visible and intersection counts -- must equal the oracle's
bit for bit (the arithmetic contract); the seeded pytest cases fix a few dozen inputs, this draws the rest:

  scene      n in {1 .. 120 000}, splat scale over two decades, opacity bands, depth planes (ties), SH degree 0..3,
             final RGB + 3x3 covariances (Door B's input, degree -1), 0 - 200 link groups with random rigid poses; one case in
             sixteen is large (up to 1M Gaussians, up to 1920x1080); one in twelve is POISONED (NaN, +-Inf, 1e+-30, 0 written over
             1 % of the means / scales / quaternions / opacities / colours)
  camera     ragged image sizes from 17x17, strips of one tile row / column thousands of pixels long, focal length (now and then
             fish-eye-short or telescope-long), radius (a camera INSIDE the cloud crosses the near plane), principal points off
             centre or outside the image, a view matrix that is not quite a rotation
  entry      one blocking frame, a batch of 2-3 views (the pair projection), a batch with one pose set per view, host-delivered
             uint8 frames, a blocking frame with the complete sorted lists kept, and PIPELINED steps (3-6 steps enqueued without waiting -- single frames or batches, new group poses
             before every step, four frames in flight over the slot ring -- then one wait); depth fill on or off; nerfstudio's eval background or a drawn one

    python tests/tools/oracle_fuzz.py [n_seeds] [first_seed] [poison-all]         (exit code 1 on the first difference; prints each case)

  meshes     `--meshes`: every case also gets 1-60 triangles (draw_mesh_case), and the frames are held to oracle.mesh_ref + the
             depth-limited oracle on the pixels the reference calls stable (oracle/mesh_ref.py); the excluded share is printed

    python tests/tools/oracle_fuzz.py --meshes [n_seeds] [first_seed]

The entry points this tool does not draw -- render_rgbd's points and mask, render_cameras_host, label frames, label lifting, point clouds --
are drawn by tests/tools/obs_fuzz.py, from the recipes below (shape_scene, poison_scene, draw_strip, draw_camera).

Test infrastructure: lives under tests/ because it calls the oracle (the checker)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402
from sim_a_splat_amd.synthetic import (NERFSTUDIO_EVAL_BACKGROUND as BG, Camera, intrinsics, look_at_viewmat, make_scene,  # noqa: E402
                                       random_group_poses)

KEYS = ("rgb", "alpha", "depth", "rgb8")


BAD_VALUES = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-30, 0.0, 3e6, 1e12, -1.0], np.float32)


# ---- the recipes of a drawn case: draw_case below and tests/tools/obs_fuzz.py draw from them, each from generator streams of its own
def shape_scene(rng, sc) -> None:
    """Opacity bands, now and then depth planes (crowded buckets, ties) and everything in a few tiles (long lists); in place."""
    lo = float(rng.choice([0.004, 0.05, 0.5]))
    sc.opacities[:] = np.clip(sc.opacities, lo, min(1.0, lo * 20 + 0.01)).astype(np.float32)
    if rng.random() < 0.25:
        sc.means[:, 2] = np.round(sc.means[:, 2] * 4) / 4                    # depth planes: crowded buckets, ties
    if rng.random() < 0.15:
        sc.means *= np.float32(0.05)                                         # everything in a few tiles: long lists


def draw_strip(rng, long_w=(1000, 4000), long_h=(1000, 3000)):
    """(W, H) of a strip: one row or one column of tiles, thousands of pixels long."""
    return (int(rng.integers(*long_w)), int(rng.integers(1, 17))) if rng.random() < 0.5 else (int(rng.integers(1, 17)), int(rng.integers(*long_h)))


def poison_scene(rng, sc) -> None:
    """Non-finite and absurd values in ~1 % of the Gaussians, in place: both sides must cull or clamp them the same way, and the
    device must not leave its buffers (the bounds-checked build counts)."""
    for arr in (sc.means, sc.scales, sc.quats, sc.opacities, sc.sh):
        flat = arr.reshape(-1)
        k = max(1, flat.size // 100)
        flat[rng.integers(0, flat.size, size=k)] = BAD_VALUES[rng.integers(0, BAD_VALUES.size, size=k)]


RADII = (0.3, 1.0, 3.0, 3.0, 6.0)                                            # 0.3 / 1.0: inside the cloud


def draw_camera(rng, W: int, H: int, odd: list = None) -> Camera:
    """One camera on a ring around the cloud, looking at its centre; one in ten is odd (``odd``, a list, is told which: it
    receives True or False)."""
    radius = float(rng.choice(RADII))
    yaw, elev = float(rng.uniform(0, 2 * np.pi)), float(rng.uniform(-0.8, 0.8)) * radius
    eye = (radius * np.sin(yaw), elev, radius * np.cos(yaw))
    f = float(rng.uniform(0.4, 1.5)) * W
    cx, cy = W / 2.0 + float(rng.uniform(-0.2, 0.2)) * W, H / 2.0 + float(rng.uniform(-0.2, 0.2)) * H
    V = look_at_viewmat(eye)
    is_odd = bool(rng.random() < 0.1)
    if is_odd:                                                           # odd cameras: fish-eye-short or telescope-long focal lengths, the
        f = float(rng.choice([0.03, 0.1, 8.0, 40.0])) * max(W, H)        # principal point outside the image, a view matrix that is not quite a rotation
        cx, cy = float(rng.uniform(-1.0, 2.0)) * W, float(rng.uniform(-1.0, 2.0)) * H
        V = V.copy(); V[:3, :3] *= np.float32(rng.uniform(0.97, 1.03))
    if odd is not None:
        odd.append(is_odd)
    return Camera(V, intrinsics(f, f * float(rng.uniform(0.8, 1.25)), cx, cy), W, H)


def draw_case(seed: int, poison_all: bool = False) -> dict:
    rng = np.random.default_rng(77_000 + seed)
    n = int(rng.choice([1, 7, 50, 800, 6000, 30000, 120000], p=[0.04, 0.06, 0.1, 0.25, 0.25, 0.2, 0.1]))
    ls = float(rng.uniform(np.log(0.003), np.log(0.3)))
    n_groups = int(rng.choice([0, 0, 0, 3, 3, 7, 7, 40, 200]))      # (40, 200: beyond the pose rows a launch carries in its arguments)
    sc = make_scene(n, seed=88_000 + seed, log_scale_mean=ls, n_groups=n_groups)
    shape_scene(rng, sc)
    deg = int(rng.choice([-1, 0, 1, 2, 3, 3, 3]))
    W, H = int(rng.integers(17, 420)), int(rng.integers(17, 300))
    if rng.random() < 0.05:                                                  # a strip: one row or one column of tiles, thousands of pixels long
        W, H = draw_strip(rng)
    poisoned = bool(rng.random() < 0.08) or poison_all
    if rng.random() < 0.06:                                                  # now and then a large frame and a large scene
        W, H = int(rng.integers(640, 1921)), int(rng.integers(480, 1081))
        n = int(rng.choice([120000, 500000, 1000000]))
        sc = make_scene(n, seed=88_000 + seed, log_scale_mean=float(rng.uniform(np.log(0.004), np.log(0.03))), n_groups=n_groups)
    if poisoned:
        poison_scene(rng, sc)
    n_views = int(rng.choice([1, 1, 2, 3]))
    cams = [draw_camera(rng, W, H) for _ in range(n_views)]
    entry = "single" if n_views == 1 else str(rng.choice(["batch", "batch", "posed", "host"]))
    if n_groups == 0 and entry == "posed":
        entry = "batch"
    bg = BG if rng.random() < 0.5 else tuple(float(v) for v in rng.uniform(0, 1, size=3).astype(np.float32))
    full_sort = bool(entry == "single" and rng.random() < 0.15)       # complete sorted lists kept (the T4/T5 arrays' path)
    steps = 1
    if rng.random() < 0.2:
        entry, steps = "pipelined", int(rng.integers(3, 7))
    poses = [random_group_poses(n_groups, seed=99_000 + 7 * seed + v, max_angle=0.6, max_shift=0.3) for v in range(max(n_views, steps))] if n_groups else None
    if entry == "pipelined":     # every step looks from its own place
        yaw0 = float(rng.uniform(0, 2 * np.pi))
        step_cams = []
        for s_ in range(steps):
            row = []
            for v in range(n_views):
                a = yaw0 + 0.7 * s_ + 2.1 * v
                row.append(Camera(look_at_viewmat((3.0 * np.sin(a), 0.3 * s_ - 0.5, 3.0 * np.cos(a))), cams[v].K, W, H))
            step_cams.append(row)
        return dict(seed=seed, scene=sc, deg=deg, n_groups=n_groups, cams=cams, entry=entry, poses=poses, fill=bool(rng.random() < 0.5), W=W, H=H,
                    steps=steps, step_cams=step_cams, bg=bg, full_sort=False, poisoned=poisoned)
    return dict(seed=seed, scene=sc, deg=deg, n_groups=n_groups, cams=cams, entry=entry, poses=poses, fill=bool(rng.random() < 0.5), W=W, H=H, bg=bg,
                full_sort=full_sort, poisoned=poisoned)


def scene_inputs(c: dict) -> dict:
    """What both sides are handed: SH coefficients cut to the degree, or final RGB + covariances (degree -1)."""
    sc, deg = c["scene"], c["deg"]
    if deg >= 0:
        return dict(colors=np.ascontiguousarray(sc.sh[:, :(deg + 1) ** 2]), quats=sc.quats, scales=sc.scales, cov=None, cov6=None)
    rng = np.random.default_rng(55_000 + c["seed"])
    q = sc.quats / np.linalg.norm(sc.quats, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * sc.scales[:, None, :]
    cov = (M @ M.transpose(0, 2, 1)).astype(np.float32)
    cov = ((cov + cov.transpose(0, 2, 1)) * np.float32(0.5)).astype(np.float32)
    cov6 = np.ascontiguousarray(np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1))
    colors = rng.uniform(0, 1, size=(sc.means.shape[0], 3)).astype(np.float32)
    if c["poisoned"]:
        flat = colors.reshape(-1)
        k = max(1, flat.size // 100)
        flat[rng.integers(0, flat.size, size=k)] = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)[rng.integers(0, 5, size=k)]
    return dict(colors=colors, quats=None, scales=None, cov=cov, cov6=cov6)


def pose_per_view(c: dict) -> list:
    """The pose rows each view is rendered with (None: a scene without groups): its own set in a posed batch, else the first."""
    n = len(c["cams"])
    if not c["poses"]:
        return [None] * n
    return list(c["poses"][:n]) if c["entry"] == "posed" else [c["poses"][0]] * n


def render_views(r, c: dict) -> list:
    """The case's views through its entry point (single, batch, posed, host), one dict of outputs per view; the scene is uploaded."""
    cams, W, H, fill, BG = c["cams"], c["W"], c["H"], c["fill"], c["bg"]
    Vs, Ks = np.stack([cm.viewmat for cm in cams]), np.stack([cm.K for cm in cams])
    if c["poses"] and c["entry"] != "posed":
        r.set_group_poses(c["poses"][0])
    if c["entry"] == "single":
        o = r.render(Vs[0], Ks[0], W, H, BG, want=KEYS, depth_fill_max=fill, full_sort=c["full_sort"])
        return [{k: v.cpu().numpy() for k, v in o.items()}]
    if c["entry"] == "host":
        frames = r.render_batch_host(Vs, Ks, W, H, BG).numpy()
        return [{"rgb8": frames[i]} for i in range(len(cams))]
    kw = dict(pose_sets=np.stack(c["poses"]), pose_set=list(range(len(cams)))) if c["entry"] == "posed" else {}
    o = r.render_batch(Vs, Ks, W, H, BG, want=KEYS, depth_fill_max=fill, **kw)
    return [{k: v[i].cpu().numpy() for k, v in o.items()} for i in range(len(cams))]


def run_case(r, c: dict) -> list:
    """Renders the case on the GPU through its entry point and with the oracle view by view; returns the differences found."""
    sc, cams, W, H, fill, BG = c["scene"], c["cams"], c["W"], c["H"], c["fill"], c["bg"]
    inp = scene_inputs(c)
    gid = sc.group_id if c["n_groups"] else None
    r.upload(sc.means, sc.opacities, inp["colors"], quats=inp["quats"], scales=inp["scales"], covariances=inp["cov"], sh_degree=c["deg"],
             group_id=gid, n_groups=c["n_groups"])
    if c["entry"] == "pipelined":
        return run_pipelined(r, c, inp, gid)
    got, view_pose = render_views(r, c), pose_per_view(c)
    diffs = []
    for i, cm in enumerate(cams):
        ref = oracle.render(sc.means, sc.opacities, inp["colors"], cm.viewmat, cm.K, W, H, quats=inp["quats"], scales=inp["scales"], cov6=inp["cov6"],
                            sh_degree=c["deg"], group_id=gid, group_Rt=view_pose[i], background=BG, depth_mode=1 if fill else 0, want_rgb8=True)
        for k, g in got[i].items():
            if not np.array_equal(g, ref[k], equal_nan=g.dtype != np.uint8):
                d = np.abs(g.astype(np.float64) - ref[k].astype(np.float64))
                diffs.append(f"view {i} {k}: {int((d > 0).sum())} values differ, max {d.max():.3e}")
        if c["entry"] == "single":
            st = r.stats()
            if st["n_visible"] != ref["n_visible"] or st["n_isect"] != ref["n_isect"]:
                diffs.append(f"counts: visible {st['n_visible']} / {ref['n_visible']}, intersections {st['n_isect']} / {ref['n_isect']}")
    return diffs


def run_pipelined(r, c: dict, inp: dict, gid) -> list:
    """c['steps'] steps enqueued back to back (block=False), each into its own output tensors and after its own set_group_poses; one
    wait at the end; then every frame of every step against the oracle."""
    import torch
    W, H, fill, sc, BG = c["W"], c["H"], c["fill"], c["scene"], c["bg"]
    outs = []
    for s_ in range(c["steps"]):
        row = c["step_cams"][s_]
        if c["poses"]:
            r.set_group_poses(c["poses"][s_])
        if len(row) == 1:
            o = r.render(row[0].viewmat, row[0].K, W, H, BG, want=KEYS, depth_fill_max=fill, block=False)
            outs.append({k: v[None] for k, v in o.items()})
        else:
            outs.append(r.render_batch(np.stack([cm.viewmat for cm in row]), np.stack([cm.K for cm in row]), W, H, BG, want=KEYS, depth_fill_max=fill,
                                       block=False))
    r.wait()
    torch.cuda.synchronize()
    diffs = []
    for s_ in range(c["steps"]):
        for i, cm in enumerate(c["step_cams"][s_]):
            ref = oracle.render(sc.means, sc.opacities, inp["colors"], cm.viewmat, cm.K, W, H, quats=inp["quats"], scales=inp["scales"], cov6=inp["cov6"],
                                sh_degree=c["deg"], group_id=gid, group_Rt=c["poses"][s_] if c["poses"] else None, background=BG,
                                depth_mode=1 if fill else 0, want_rgb8=True)
            for k in KEYS:
                g = outs[s_][k][i].cpu().numpy()
                if not np.array_equal(g, ref[k], equal_nan=g.dtype != np.uint8):
                    d = np.abs(g.astype(np.float64) - ref[k].astype(np.float64))
                    diffs.append(f"step {s_} view {i} {k}: {int((d > 0).sum())} values differ, max {d.max():.3e}")
    return diffs


# ---- meshes -----------------------------------------------------------------------------------------------------------------
# The seeds the suite runs (test_gpu_d_oracle_fuzz.py): from 0 upward, skipping those whose excluded share, from the reference and
# the oracle alone, exceeds 10 % (one-tile-wide strips, principal points far outside the image).  tests/test_mesh_ref_cpu.py
# recomputes the list and asserts that no more than 5 of the first 45 seeds were skipped.
MESH_FUZZ_SEEDS = tuple(range(40))
MESH_MAX_EXCLUDED = 0.10
# Found by `--meshes 400`: with a finite vertex at z = 1e30 as the inside end of an edge that crosses the near plane, k_mesh_setup's
# cut i + s (o - i) cancelled to rounding noise and the clipped corner landed at the principal point (seeds 61, 161, 181; fixed:
# the edge is cut from its end nearer the plane).  Seeds 177, 213, 387 are far vertices that the kernel always drew right and
# the reference's first formulation did not.  Seeds 163, 279: the far vertex is the triangle's first, the shading normal's two edges
# from it cancelled to exactly zero and the triangle was dropped as degenerate (fixed: the edges that leave the vertex nearest the
# origin).  All eight are kept as named cases.
MESH_SEEDS_VERTEX_AT_1E30 = (61, 161, 181, 163, 279, 177, 213, 387)


def draw_mesh_case(seed: int, poison_all: bool = False) -> dict:
    """draw_case(seed) plus, from a generator stream of its own, 1-60 triangles drawn in the first camera's space (the coverage
    test's recipe: some across the near plane, some beyond the frame, a split quad, and a few large tilted ones through the cloud),
    colours, ka / kd, and now and then a pose group.  Entry points: single, batch, posed, host (the pipelined arm becomes a single
    frame or a batch: non-blocking mesh frames have a fixed case in test_gpu_h_mesh_oracle.py).  One case in eight has poisoned
    vertices (NaN, +-Inf, 1e30): such triangles are dropped, in the reference too."""
    import mesh_cases as mc
    c = draw_case(seed, poison_all)
    rng = np.random.default_rng(66_000 + seed)
    if c["entry"] == "pipelined":
        c["entry"] = "single" if len(c["cams"]) == 1 else "batch"
    cm = c["cams"][0]
    W, H = c["W"], c["H"]
    V, K = np.asarray(cm.viewmat, np.float64).reshape(4, 4), np.asarray(cm.K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    dist = float(np.linalg.norm(np.linalg.solve(V[:3, :3], V[:3, 3])))          # the camera's distance from the cloud's centre
    n = int(rng.integers(1, 61))
    tri = []                                                                     # camera-space triangles [3,3]
    for _ in range(int(rng.integers(0, 3))):                                     # large tilted planes through the cloud
        za, zb = sorted(rng.uniform(max(0.2, dist - 1.0), dist + 1.0, 2))
        uv = np.array([[-20.0, -20.0], [W + 20.0, -20.0], [W + 20.0, H + 20.0], [-20.0, H + 20.0]])
        w = 1.0 / za + (1.0 / zb - 1.0 / za) * (rng.uniform(0.2, 0.8) * uv[:, 0] / W + rng.uniform(0.2, 0.8) * uv[:, 1] / H)
        z = 1.0 / np.maximum(w, 1e-3)
        q = np.stack([(uv[:, 0] - cx) * z / fx, (uv[:, 1] - cy) * z / fy, z], 1)
        tri += [q[[0, 1, 2]], q[[0, 2, 3]]]
    d = float(rng.uniform(0.5, dist + 1.0))                                      # a split quad, flat in depth
    uv = np.array([[0.3 * W, 0.2 * H], [0.7 * W, 0.2 * H], [0.7 * W, 0.8 * H], [0.3 * W, 0.8 * H]])
    q = np.stack([(uv[:, 0] - cx) * d / fx, (uv[:, 1] - cy) * d / fy, np.full(4, d)], 1)
    tri += [q[[0, 1, 2]], q[[0, 2, 3]]]
    k = 0
    while len(tri) < n:
        zc = rng.uniform(0.3, dist + 2.0)
        u, v = rng.uniform(-0.3 * W, 1.3 * W, 3), rng.uniform(-0.3 * H, 1.3 * H, 3)
        z = zc + rng.uniform(-0.4, 0.4, 3)
        if k % 7 == 0:
            z[0] = -0.5                                                          # crosses the near plane
        tri.append(np.stack([(u - cx) * np.abs(z) / fx, (v - cy) * np.abs(z) / fy, z], 1))
        k += 1
    order = rng.permutation(len(tri))[:n]
    pc = np.concatenate([tri[i] for i in order])
    world = np.linalg.solve(V[:3, :3], (pc - V[:3, 3]).T).T
    T = len(order)
    groups = None
    if c["n_groups"] and rng.random() < 0.5:
        g = int(rng.integers(0, c["n_groups"]))
        world, groups = mc.to_group_local(world, c["poses"][0][g]), np.full(T, g, np.uint8)
    verts = np.ascontiguousarray(world, dtype=np.float32)
    poisoned_vertices = bool(rng.random() < 0.125)
    if poisoned_vertices:
        flat = verts.reshape(-1)
        kk = int(rng.integers(1, 4))
        flat[rng.integers(0, flat.size, size=kk)] = np.array([np.nan, np.inf, -np.inf, 1e30], np.float32)[rng.integers(0, 4, size=kk)]
    ka, kd = (0.4, 0.6) if rng.random() < 0.5 else (float(rng.uniform(0.0, 1.0)), float(rng.uniform(0.0, 1.0)))
    c["mesh"] = dict(verts=verts, tris=np.arange(3 * T, dtype=np.int32).reshape(T, 3), cols=rng.uniform(0, 1, size=(T, 3)).astype(np.float32),
                     groups=groups, ka=ka, kd=kd, poisoned_vertices=poisoned_vertices)
    c["full_sort"] = False
    return c


def as_case(c: dict) -> dict:
    """A drawn mesh case in mesh_cases' form: every view, with the pose rows its entry point renders it with."""
    import mesh_cases as mc
    s, inp, m, G = c["scene"], scene_inputs(c), c["mesh"], c["n_groups"]
    sc = dict(means=s.means, op=s.opacities, colors=inp["colors"], sh=c["deg"], quats=inp["quats"], scales=inp["scales"], cov6=inp["cov6"],
              gid=s.group_id if G else None, G=G, Rt=np.asarray(c["poses"][0], np.float32).reshape(-1, 12) if G else None)
    return dict(sc=sc, cams=[(np.asarray(cm.viewmat, np.float32), np.asarray(cm.K, np.float32), c["W"], c["H"]) for cm in c["cams"]],
                mesh=mc._mesh(m["verts"], m["tris"], m["cols"], m["groups"], m["ka"], m["kd"]), bg=tuple(float(v) for v in c["bg"]),
                poses=pose_per_view(c) if G else None, describe=describe_mesh(c))


def mesh_reference(c: dict, i: int, want_frame: bool = True) -> dict:
    """View i of a mesh case from the reference and the oracle alone: stable mask, excluded and covered share and (want_frame) the frame."""
    import mesh_cases as mc
    e = mc.expected(as_case(c), i, want_frame=want_frame)
    return {k: e[k] for k in ("stable", "excluded", "covered") + (("frame",) if want_frame else ())}


def mesh_excluded_share(c: dict) -> float:
    return max(mesh_reference(c, i, want_frame=False)["excluded"] for i in range(len(c["cams"])))


def run_mesh_case(r, c: dict):
    """Renders the mesh case on the GPU through its entry point; returns (differences on stable pixels, largest excluded share)."""
    import mesh_cases as mc
    case = as_case(c)
    mc.upload_case(r, case)
    got = render_views(r, c)
    diffs, excluded = [], 0.0
    for i in range(len(got)):
        e = mc.expected(case, i)
        excluded = max(excluded, e["excluded"])
        diffs += [f"view {i} {d}" for d in mc.compare(got[i], e, fill=c["fill"], bits=False)[0]]
    return diffs, excluded


def describe_mesh(c: dict) -> str:
    m = c["mesh"]
    return describe(c) + (f" | triangles={len(m['tris'])} group={'-' if m['groups'] is None else int(m['groups'][0])} ka={m['ka']:.2f} kd={m['kd']:.2f}"
                          f"{' POISONED VERTICES' if m['poisoned_vertices'] else ''}")


def describe(c: dict) -> str:
    return (f"seed {c['seed']}: n={c['scene'].means.shape[0]} degree={c['deg']} groups={c['n_groups']} {c['W']}x{c['H']} views={len(c['cams'])} "
            f"entry={c['entry']}{'x%d' % c['steps'] if c['entry'] == 'pipelined' else ''} fill={c['fill']}{' full_sort' if c['full_sort'] else ''}{'' if c['bg'] is BG else ' bg=drawn'}{' POISONED' if c['poisoned'] else ''}")


def main(argv) -> int:
    from sim_a_splat_amd.rasterizer import Rasterizer
    meshes = "--meshes" in argv
    argv = [a for a in argv if a != "--meshes"]
    n_seeds = int(argv[1]) if len(argv) > 1 else 60
    first = int(argv[2]) if len(argv) > 2 else 0
    poison_all = len(argv) > 3 and argv[3] == "poison-all"
    r = Rasterizer(0)
    bad = 0
    for seed in range(first, first + n_seeds):
        if meshes:
            c = draw_mesh_case(seed, poison_all)
            diffs, excluded = run_mesh_case(r, c)
            print(describe_mesh(c), f"excluded={100 * excluded:.2f} % ->", "bit-equal on stable pixels" if not diffs else "DIFFERENT: " + "; ".join(diffs),
                  flush=True)
            bad += bool(diffs)
            continue
        c = draw_case(seed, poison_all)
        diffs = run_case(r, c)
        st = r.stats()
        print(describe(c), f"max_list={st['max_tile_len']} ->", "bit-equal" if not diffs else "DIFFERENT: " + "; ".join(diffs), flush=True)
        bad += bool(diffs)
    from sim_a_splat_amd import _capi
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):      # the bounds-checked build (SAS_LIB_PATH=variants/lib_bounds.so): every computed index was range-checked
        import ctypes
        out = (ctypes.c_uint64 * 4)()
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.sas_debug_bounds(out, 0)
        print(f"bounds-checked build: {out[0]} out-of-range accesses" + (f" (first: code {out[1]}, index {out[2]}, limit {out[3]})" if out[0] else ""))
        bad += int(out[0] != 0)
    r.close()
    print(f"{n_seeds} {'mesh ' if meshes else ''}cases from seed {first}: " +
          (("every output bit-equal to the reference on its stable pixels" if meshes else "every output bit-equal to the oracle") if bad == 0
           else f"{bad} cases differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
