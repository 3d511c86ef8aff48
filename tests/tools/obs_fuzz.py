"""Differential fuzzer of the OBSERVATION entry points: what oracle_fuzz.py does for render / render_batch / render_batch_host, for the
consumers behind the frame -- RGB-D points and mask, the in-library camera algebra, label frames, label lifting, point clouds.  Every
expectation comes from the C oracle, tests/tools/cloud_ref.py, tests/tools/lift_ref.py and NumPy; nothing expected is a GPU output.
Scenes and cameras are oracle_fuzz.py's recipes (shape_scene, poison_scene, draw_strip, draw_camera) at sizes of this tool's own,
drawn from generator streams of its own; a case is a function of its seed.

  scene      n in {1, 7, 50, 150, 800, 3000}, splat scale over two decades, opacity bands, depth planes (ties), everything in a few
             tiles, SH degree -1..3 (scene_inputs), ALWAYS groups: G in {1, 3, 7, 8, 9, 40} with random rigid poses (8, 9, 40 cross
             the label kernel's 8-channel chunk edge), three pose sets; one case in eight is POISONED
  camera     1-3 views of draw_camera (inside the cloud, fx != fy, principal points off centre, one in ten odd), W, H in 17..200,
             one case in ten a strip of 1000-3000 px by 1-16 px (either orientation); eval background or a drawn one; depth fill drawn
  arm        one per case, drawn (lift only where n <= lift_ref.ORACLE_MAX):
    rgbd          Rasterizer.render_rgbd per view, max_depth None / 1.0 / drawn inside the oracle depth's range: rgb, alpha, depth =
                  oracle.render, points and mask = oracle.unproject of the oracle's depth
    cameras_host  render_cameras_host with drawn camera-to-world poses and a vertical fov of 20-120 degrees: the oracle's rgb8 at
                  SplatScene._views_and_Ks' view matrices and intrinsics
    labels        render_batch_labels(want=labels, rgb8, depth), min_alpha in {0, 0.5, 1, uniform}, pose sets for several views:
                  labels = label_rule(w, a), w the oracle's frames of the scene recoloured one-hot by group (three groups per
                  frame, sh_degree -1, background 0), a the oracle's alpha; rgb8 and depth = the oracle's
    lift          lift_labels on the views with drawn label images (uniform per pixel, constant on 4x4 blocks, the case's own
                  expected label frame), n_labels in {1, G, 256}, one case in four accumulated over two calls:
                  (votes, seen) = lift_ref.sums over lift_ref.weights_oracle, exact int64
    cloud         render_batch_labels' device tensors fed to sample_point_cloud (stride, K, keep_labels, bounds, voxel grid, frame,
                  one cloud or one per view drawn): cloud_ref.cloud32 fed the ORACLE's depth and rgb8 and the reference labels;
                  the three frame outputs are held to the oracle as well, so a cloud mismatch can be told from a frame mismatch

    python tests/tools/obs_fuzz.py [n_seeds] [first_seed] [poison-all]         (exit code 1 on any difference; prints each case)

Test infrastructure: lives under tests/ because it calls the oracle (the checker)."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cloud_ref  # noqa: E402
import lift_ref  # noqa: E402
import oracle_fuzz as fz  # noqa: E402
import oracle  # noqa: E402  (oracle_fuzz put the repository root on the path)
from sim_a_splat_amd.synthetic import make_scene, random_group_poses  # noqa: E402

ARMS = ("rgbd", "cameras_host", "labels", "lift", "cloud")
SIZES = (1, 7, 50, 150, 800, 3000)
GROUPS = (1, 3, 7, 8, 9, 40)
POSE_SETS = 3
# The cases the suite runs (tests/test_gpu_q_obs_fuzz.py), per arm: seeds that draw the arm, picked from the first 500 so that the
# conditions of tests/test_obs_fuzz_cpu.py hold (a poisoned scene, a strip and an odd camera per arm; labels: G = 9 and 40, min_alpha
# 0 over untouched pixels and 1; lift: 256 labels with 255 present, Gaussians nothing sees, two calls into one buffer; cloud: no
# survivor, fewer than K, more than K, more than the sampling kernel keeps resident, a grid that thins, a crop that removes) --
# settled there from the references alone, before anything runs on a GPU.
OBS_SEEDS = {
    "rgbd": (6, 11, 16, 19, 26, 33, 36, 37, 40, 52, 57, 73),
    "cameras_host": (2, 3, 5, 15, 18, 30, 60, 72, 87, 99, 133, 158),
    "labels": (0, 8, 9, 22, 55, 80, 82, 84, 144, 166, 182, 394),
    "lift": (1, 10, 12, 14, 35, 85, 102, 248, 396, 435, 449, 497),
    "cloud": (4, 7, 20, 44, 59, 66, 83, 105, 116, 136, 181, 271),
}


# Found by `obs_fuzz.py 1500` (seeds 421, 695) and `obs_fuzz.py 100 6000 poison-all` (seed 6057), as (seed, poison_all): `seen` of
# one Gaussian too large by 0.999 x 2^32 per lane of its tiles that lies beyond W or H.  The Gaussian's opacity is NaN or +Inf: its alpha,
# fminf(0.999, opacity x E), is 0.999 whatever sigma is, so the lanes parked outside the image (x = NaN, T = 1) composited it, and
# k_lift_labels summed `seen` over all 16 lanes of a block (votes were right: those lanes carry label 256).  Fixed: such a lane gives
# nothing.  reduced_lift_case() is the same with two Gaussians at 17 x 17.
LIFT_SEEDS_OPACITY_NOT_FINITE = ((421, False), (695, False), (6057, True))


def reduced_lift_case(opacity=np.inf):
    """(scene, camera, labels [1,17,17], n_labels) in lift_ref's form: two Gaussians in front of a 17 x 17 camera (four tiles, three
    of them with 15 of their 16 columns or rows beyond the image), the second with the given opacity and a footprint over all four."""
    import scene_cases as sc_kit
    sc = lift_ref.blob_scene(2, seed=3, scale=0.2, spread=0.3, z_spread=0.3)
    sc["op"][1] = opacity
    sc["scales"][1] = 1.0
    labels = np.random.default_rng(4).integers(0, 2, size=(1, 17, 17)).astype(np.uint8)
    return sc, sc_kit.ring(17, 17, f=20.0), labels, 2


# ---- the draw ------------------------------------------------------------------------------------------------------------------------------
def draw_case(seed: int, poison_all: bool = False) -> dict:
    """Scene, cameras and arm of a seed (stream 177 000 + seed) and the arm's own parameters (stream 188 000 + seed).  What an arm can
    only draw once its references exist -- a max_depth inside the depth's range, a crop box around the uncropped points -- is kept
    as a uniform number here and turned into the value by reference()."""
    rng = np.random.default_rng(177_000 + seed)
    n = int(rng.choice(SIZES, p=[0.05, 0.1, 0.2, 0.2, 0.25, 0.2]))
    ls = float(rng.uniform(np.log(0.003), np.log(0.3)))
    G = int(rng.choice(GROUPS))
    sc = make_scene(n, seed=288_000 + seed, log_scale_mean=ls, n_groups=G)
    fz.shape_scene(rng, sc)
    deg = int(rng.choice([-1, 0, 1, 2, 3, 3, 3]))
    W, H = int(rng.integers(17, 201)), int(rng.integers(17, 201))
    strip = bool(rng.random() < 0.1)
    if strip:
        W, H = fz.draw_strip(rng, (1000, 3001), (1000, 3001))
    poisoned = bool(rng.random() < 0.125) or poison_all
    if poisoned:
        fz.poison_scene(rng, sc)
    n_views = int(rng.integers(1, 4))
    odd = []
    cams = [fz.draw_camera(rng, W, H, odd) for _ in range(n_views)]
    bg = fz.BG if rng.random() < 0.5 else tuple(float(v) for v in rng.uniform(0, 1, size=3).astype(np.float32))
    fill = bool(rng.random() < 0.5)
    arm = str(rng.choice([a for a in ARMS if a != "lift" or n <= lift_ref.ORACLE_MAX]))
    poses = np.stack([random_group_poses(G, seed=299_000 + 7 * seed + s, max_angle=0.6, max_shift=0.3) for s in range(POSE_SETS)])
    c = dict(seed=seed, scene=sc, deg=deg, n_groups=G, cams=cams, W=W, H=H, bg=bg, fill=fill, poisoned=poisoned, strip=strip,
             odd=any(odd), arm=arm, poses=poses)
    c["par"] = _ARM_DRAWS[arm](np.random.default_rng(188_000 + seed), c)
    return c


def _draw_pose_sets(rng, c) -> dict:
    """Several views: a pose set per view, drawn from the case's three (pose_sets + pose_set); one view: the context's poses (set 0)."""
    C = len(c["cams"])
    return dict(pose_set=[int(s) for s in rng.integers(0, POSE_SETS, size=C)] if C > 1 else None,
                min_alpha=float([0.0, 0.5, 1.0, float(rng.uniform(0, 1))][int(rng.integers(0, 4))]))


def _draw_rgbd(rng, c) -> dict:
    return dict(kind=str(rng.choice(["none", "one", "inside"])), u=[float(v) for v in rng.uniform(0, 1, size=len(c["cams"]))])


def _draw_cameras_host(rng, c) -> dict:
    """Camera-to-world poses (OpenCV axes): a position at draw_camera's radii in a drawn direction; three in four look at the cloud's
    centre and are then turned by up to 0.6 rad about a drawn axis, one in four looks anywhere.  wxyz is rounded to float32."""
    from sim_a_splat_amd import poses as P
    from sim_a_splat_amd.synthetic import look_at_viewmat
    C = int(rng.integers(1, 4))
    q, p = np.zeros((C, 4)), np.zeros((C, 3))
    for i in range(C):
        d = rng.normal(size=3)
        d[1] *= 0.5
        p[i] = float(rng.choice(fz.RADII)) * d / np.linalg.norm(d)
        axis, angle = rng.normal(size=3), float(rng.uniform(-0.6, 0.6))
        if rng.random() < 0.25:
            wxyz = rng.normal(size=4)
        else:
            R = np.asarray(look_at_viewmat(tuple(p[i])), np.float64)[:3, :3].T @ P.quat_wxyz_to_matrix(
                np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * axis / np.linalg.norm(axis)]))
            wxyz = P.matrix_to_quat_wxyz(R)
        q[i] = (wxyz / np.linalg.norm(wxyz)).astype(np.float32)
    return dict(wxyz=q, position=p, fov=float(np.deg2rad(rng.uniform(20.0, 120.0))))


def _draw_label_images(rng, c, C) -> list:
    """One recipe per view, (kind, a seed of its own): "uniform" per pixel over {0..G-1, 255}, "blocks" constant on 4x4 blocks (the
    vote loop's one-turn path), "frame" the case's own expected label frame (the seed unused)."""
    return [(("uniform", "blocks", "frame")[int(rng.integers(0, 3))], int(rng.integers(0, 2 ** 31))) for _ in range(C)]


def _draw_lift(rng, c) -> dict:
    C = len(c["cams"])
    return dict(n_labels=int(rng.choice([1, c["n_groups"], 256])), images=_draw_label_images(rng, c, C),
                again=_draw_label_images(rng, c, C) if rng.random() < 0.25 else None)


def _draw_cloud(rng, c) -> dict:
    C, G = len(c["cams"]), c["n_groups"]
    par = _draw_pose_sets(rng, c)
    keep = None
    if rng.random() < 0.5:
        keep = sorted({int(g) for g in rng.integers(0, G, size=int(rng.integers(1, G + 1)))} | ({255} if rng.random() < 0.4 else set()))
    crop = bool(rng.random() < 0.5)
    frame = None
    kind = str(rng.choice(["none", "rigid", "affine"]))
    if kind != "none":
        frame = np.eye(4)
        frame[:3, 3] = rng.uniform(-0.5, 0.5, size=3)
        if kind == "rigid":
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            frame[:3, :3] = q * np.sign(np.linalg.det(q))
        else:
            frame[:3, :3] = np.eye(3) + rng.uniform(-0.4, 0.4, size=(3, 3))
    par.update(stride=int(rng.integers(1, 4)), K=int(rng.choice([1, 64, 300, 1500])), keep=keep, crop=crop,
               voxel=bool(crop and rng.random() < 0.5), frame=frame, frame_kind=kind, per_view=bool(C > 1 and rng.random() < 0.5))
    return par


_ARM_DRAWS = dict(rgbd=_draw_rgbd, cameras_host=_draw_cameras_host, labels=_draw_pose_sets, lift=_draw_lift, cloud=_draw_cloud)


def describe(c: dict) -> str:
    par = {k: v for k, v in c["par"].items() if k not in ("wxyz", "position", "frame", "images", "again", "u")}
    if c["arm"] == "lift":
        par.update(images=[k for k, _ in c["par"]["images"]], again=None if c["par"]["again"] is None else [k for k, _ in c["par"]["again"]])
    if c["arm"] == "cameras_host":
        par.update(views=len(c["par"]["wxyz"]), fov=round(par["fov"], 4))
    return (f"seed {c['seed']} {c['arm']}: n={c['scene'].means.shape[0]} degree={c['deg']} groups={c['n_groups']} {c['W']}x{c['H']} "
            f"views={len(c['cams'])} fill={c['fill']}{'' if c['bg'] is fz.BG else ' bg=drawn'}{' strip' if c['strip'] else ''}"
            f"{' odd-camera' if c['odd'] else ''}{' POISONED' if c['poisoned'] else ''} | " + " ".join(f"{k}={v}" for k, v in par.items()))


# ---- references: the oracle, cloud_ref, lift_ref, NumPy ----------------------------------------------------------------------------------
def label_rule(weights, alpha, min_alpha=0.5):
    """L of DESIGN.md 3, "Label frames": the smallest g among the maxima of ``weights [..., G]``, clamped to 255, and 255 where
    ``alpha < min_alpha`` compared in float32.  uint8."""
    lab = np.minimum(np.argmax(weights, axis=-1), 255)                  # (argmax: the first of the largest)
    none = np.asarray(alpha, np.float32).reshape(lab.shape) < np.float32(min_alpha)
    return np.where(none, 255, lab).astype(np.uint8)


def _oracle(c, inp, V, K, Rt, colors=None, bg=None, fill=None):
    """One oracle frame of the case's scene at (V, K) under the pose rows Rt; ``colors [n,3]``: the scene recoloured (final RGB)."""
    sc = c["scene"]
    return oracle.render(sc.means, sc.opacities, inp["colors"] if colors is None else colors, V, K, c["W"], c["H"], quats=inp["quats"],
                         scales=inp["scales"], cov6=inp["cov6"], sh_degree=c["deg"] if colors is None else -1, group_id=sc.group_id,
                         group_Rt=Rt, background=c["bg"] if bg is None else bg, depth_mode=int(c["fill"] if fill is None else fill),
                         want_rgb8=True)


def group_weights(c, inp, V, K, Rt):
    """(w [H,W,G], alpha [H,W,1]) float32: the channels of the oracle's frames of the scene recoloured one-hot by group, three groups
    per frame, zero background; alpha is those frames' own (bit-identical to the original frame's: colours do not reach it)."""
    G, gid = c["n_groups"], np.asarray(c["scene"].group_id, np.int64)
    w, alpha = [], None
    for o in range(0, G, 3):
        fr = _oracle(c, inp, V, K, Rt, colors=(gid[:, None] == o + np.arange(3)[None, :]).astype(np.float32), bg=(0.0, 0.0, 0.0), fill=False)
        w.append(fr["rgb"])
        assert alpha is None or np.array_equal(alpha.view(np.uint32), fr["alpha"].view(np.uint32))
        alpha = fr["alpha"]
    return np.concatenate(w, -1)[..., :G], alpha


def kit_scene(c, inp) -> dict:
    """The case's scene as a scene_cases dict (what lift_ref takes)."""
    sc = c["scene"]
    return dict(means=sc.means, op=sc.opacities, colors=inp["colors"], sh=c["deg"], quats=inp["quats"], scales=inp["scales"], cov6=inp["cov6"],
                gid=sc.group_id, G=c["n_groups"], Rt=c["poses"][0])


def _view_poses(c) -> list:
    ps = c["par"].get("pose_set")
    return [c["poses"][0]] * len(c["cams"]) if ps is None else [c["poses"][s] for s in ps]


def _frames_and_labels(c, inp, want, notes, fill):
    """rgb8, depth and labels of every view of a labels / cloud case: view<i>.<name> into ``want``; returns the three stacked."""
    out = dict(rgb8=[], depth=[], labels=[])
    for i, (cm, Rt) in enumerate(zip(c["cams"], _view_poses(c))):
        fr = _oracle(c, inp, cm.viewmat, cm.K, Rt, fill=fill)
        w, a = group_weights(c, inp, cm.viewmat, cm.K, Rt)
        notes["alpha_same"] = notes.get("alpha_same", True) and np.array_equal(a.view(np.uint32), fr["alpha"].view(np.uint32))
        notes["weights_in_range"] = notes.get("weights_in_range", True) and bool(np.isfinite(w).all() and (w >= 0).all() and (w < 1).all())
        lab = label_rule(w, a, c["par"]["min_alpha"])
        notes.setdefault("untouched", []).append(int((a == 0).sum()))
        for k, v in (("rgb8", fr["rgb8"]), ("depth", fr["depth"]), ("labels", lab)):
            want[f"view{i}.{k}"] = v
            out[k].append(v)
    notes["distinct_labels"] = int(len(set(np.unique(np.stack(out["labels"])).tolist()) - {255}))
    return {k: np.stack(v) for k, v in out.items()}


def _label_images(c, inp, recipes) -> np.ndarray:
    """[C,H,W] uint8 of a lift case's recipes."""
    G, W, H = c["n_groups"], c["W"], c["H"]
    values = np.array(list(range(G)) + [255], np.uint8)
    out = []
    for (kind, seed), cm in zip(recipes, c["cams"]):
        rng = np.random.default_rng(seed)
        if kind == "uniform":
            out.append(values[rng.integers(0, len(values), size=(H, W))])
        elif kind == "blocks":
            b = values[rng.integers(0, len(values), size=((H + 3) // 4, (W + 3) // 4))]
            out.append(np.repeat(np.repeat(b, 4, axis=0), 4, axis=1)[:H, :W])
        else:
            out.append(label_rule(*group_weights(c, inp, cm.viewmat, cm.K, c["poses"][0]), 0.5))
    return np.ascontiguousarray(np.stack(out))


def reference(c: dict) -> dict:
    """dict(want, args, notes) of a case, on the CPU: ``want`` name -> array, what compare() holds the GPU's outputs to; ``args`` what
    the arm is called with and only the references could settle; ``notes`` figures about the expectation itself (how many labels,
    survivors, votes), for tests/test_obs_fuzz_cpu.py."""
    inp = fz.scene_inputs(c)
    par, cams, W, H = c["par"], c["cams"], c["W"], c["H"]
    want, args, notes = {}, {}, {}
    if c["arm"] == "rgbd":
        args["max_depth"] = []
        for i, cm in enumerate(cams):
            fr = _oracle(c, inp, cm.viewmat, cm.K, c["poses"][0])
            md = {"none": None, "one": 1.0}.get(par["kind"], 1.0)
            d = fr["depth"][np.isfinite(fr["depth"]) & (fr["depth"] > 0)]
            if par["kind"] == "inside" and d.size:
                md = float(np.float32(d.min() + par["u"][i] * (float(d.max()) - float(d.min()))))
            pts, mask = oracle.unproject(fr["depth"], cm.K, md)
            args["max_depth"].append(md)
            want.update({f"view{i}.rgb": fr["rgb"], f"view{i}.alpha": fr["alpha"], f"view{i}.depth": fr["depth"], f"view{i}.points": pts,
                         f"view{i}.mask": mask.view(np.uint8)})
            notes.setdefault("masked", []).append((int(mask.sum()), int(mask.size)))
    elif c["arm"] == "cameras_host":
        from sim_a_splat_amd.scene import SplatScene
        Vs, Ks = SplatScene._views_and_Ks(H, W, par["wxyz"], par["position"], par["fov"])
        for i in range(len(Vs)):
            fr = _oracle(c, inp, Vs[i], Ks[i], c["poses"][0])
            want[f"view{i}.rgb8"] = fr["rgb8"]
            notes.setdefault("touched", []).append(int((fr["alpha"] > 0).sum()))
    elif c["arm"] == "labels":
        _frames_and_labels(c, inp, want, notes, c["fill"])
    elif c["arm"] == "lift":
        sc = kit_scene(c, inp)
        n = len(sc["means"])
        votes, seen = np.zeros((n, par["n_labels"]), np.int64), np.zeros(n, np.int64)
        weights = [lift_ref.weights_oracle(sc, (cm.viewmat, cm.K, W, H), c["poses"][0]) for cm in cams]
        args["labels"] = [_label_images(c, inp, rec) for rec in (par["images"], par["again"]) if rec is not None]
        for labels in args["labels"]:
            for w, lab in zip(weights, labels):
                v, s = lift_ref.sums(w, lab, par["n_labels"])
                votes += v
                seen += s
        want.update(votes=votes, seen=seen)
        notes.update(has_255=bool(any((lab == 255).any() for lab in args["labels"])))
    else:
        from sim_a_splat_amd.rasterizer import cloud_keep_table, cloud_transforms
        fr = _frames_and_labels(c, inp, want, notes, c["fill"])
        C = len(cams)
        Vs, Ks = np.stack([cm.viewmat for cm in cams]), np.stack([cm.K for cm in cams])
        kw = dict(rgb8=fr["rgb8"], labels=fr["labels"], keep=cloud_keep_table(par["keep"]), stride=par["stride"],
                  clouds=list(range(C)) if par["per_view"] else None, n_clouds=C if par["per_view"] else 1)
        T = cloud_transforms(Vs, par["frame"])
        free = cloud_ref.cloud32(fr["depth"], Ks, T, 0, **kw)           # no crop, no grid, no sampling: the candidates and their count
        pts = np.concatenate(free["w"])
        bounds, voxel = None, 0.0
        if par["crop"] and len(pts):
            bounds = np.stack([np.percentile(pts, 10, axis=0), np.percentile(pts, 90, axis=0)]).astype(np.float32)
            if par["voxel"]:
                voxel = float(np.float32((bounds[1] - bounds[0]).max() / np.float32(20.0)))    # at most 21 cells a side
        args.update(bounds=bounds, voxel=voxel)
        ref = cloud_ref.cloud32(fr["depth"], Ks, T, par["K"], bounds=bounds, voxel=voxel, **kw)
        want.update({f"cloud.{k}": ref[k] for k in ("points", "index", "count", "colors", "labels")})
        notes.update(M=ref["count"].tolist(), M_free=free["count"].tolist(),
                     M_no_grid=cloud_ref.cloud32(fr["depth"], Ks, T, 0, bounds=bounds, **kw)["count"].tolist() if voxel > 0 else None)
    return dict(want=want, args=args, notes=notes)


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------------
def run_arm(r, c: dict, args: dict) -> dict:
    """The case's arm on the Rasterizer ``r``: name -> array, named as reference()'s ``want``."""
    import torch
    sc, par, cams, W, H, bg = c["scene"], c["par"], c["cams"], c["W"], c["H"], c["bg"]
    inp = fz.scene_inputs(c)
    r.upload(sc.means, sc.opacities, inp["colors"], quats=inp["quats"], scales=inp["scales"], covariances=inp["cov"], sh_degree=c["deg"],
             group_id=sc.group_id, n_groups=c["n_groups"])
    r.set_group_poses(c["poses"][0])
    Vs, Ks = np.stack([cm.viewmat for cm in cams]), np.stack([cm.K for cm in cams])
    got = {}
    if c["arm"] == "rgbd":
        for i, cm in enumerate(cams):
            o = r.render_rgbd(cm.viewmat, cm.K, W, H, bg, max_depth=args["max_depth"][i], depth_fill_max=c["fill"])
            got.update({f"view{i}.{k}": v.cpu().numpy() for k, v in o.items() if k != "mask"})
            got[f"view{i}.mask"] = o["mask"].view(torch.uint8).cpu().numpy()
        return got
    if c["arm"] == "cameras_host":
        frames = r.render_cameras_host(par["wxyz"], par["position"], par["fov"], W, H, bg).numpy()
        return {f"view{i}.rgb8": frames[i] for i in range(len(frames))}
    if c["arm"] == "lift":
        votes = seen = None
        for labels in args["labels"]:
            o = r.lift_labels(Vs, Ks, W, H, labels, par["n_labels"], votes=votes, seen=seen)
            votes, seen = o["votes"], o["seen"]
        return dict(votes=votes.cpu().numpy(), seen=seen.cpu().numpy())
    kw = dict(pose_sets=c["poses"], pose_set=par["pose_set"]) if par["pose_set"] is not None else {}
    o = r.render_batch_labels(Vs, Ks, W, H, bg, min_alpha=par["min_alpha"], want=("labels", "rgb8", "depth"), depth_fill_max=c["fill"], **kw)
    for k in ("labels", "rgb8", "depth"):
        a = o[k].cpu().numpy()
        got.update({f"view{i}.{k}": a[i] for i in range(len(cams))})
    if c["arm"] == "cloud":
        C = len(cams)
        cl = r.sample_point_cloud(o["depth"], Vs, Ks, W, H, par["K"], rgb8=o["rgb8"], labels=o["labels"], keep_labels=par["keep"],
                                  bounds=args["bounds"], voxel_size=args["voxel"], stride=par["stride"], frame=par["frame"],
                                  clouds=list(range(C)) if par["per_view"] else None, n_clouds=C if par["per_view"] else 1)
        got.update({f"cloud.{k}": v.cpu().numpy() for k, v in cl.items()})
    return got


def compare(got: dict, want: dict) -> list:
    """The differences between what an arm delivered and the expectation, one line per output that differs: float32 compared as bits
    (a NaN equals a NaN), everything else as values; how many differ, and the largest difference where a difference means something
    (not between two labels or two pixel indices)."""
    diffs = []
    for k, w in want.items():
        if k not in got:
            diffs.append(f"{k}: missing")
            continue
        g, w = np.asarray(got[k]), np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            diffs.append(f"{k}: {g.dtype}{list(g.shape)} for {w.dtype}{list(w.shape)}")
            continue
        if w.dtype == np.float32:
            bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
        else:
            bad = g != w
        if bad.any():
            line = f"{k}: {int(bad.sum())} values differ"
            if not k.endswith(("labels", "index", "mask")):
                with np.errstate(all="ignore"):
                    d = np.abs(g[bad].astype(np.float64) - w[bad].astype(np.float64))
                line += f", max {np.nanmax(d) if np.isfinite(d).any() else np.nan:.3e}"
            first = tuple(int(v) for v in np.argwhere(bad)[0])
            diffs.append(line + f" (first at {first}: {g[first]!r} for {w[first]!r})")
    return diffs


def run_case(r, c: dict) -> list:
    ref = reference(c)
    return compare(run_arm(r, c, ref["args"]), ref["want"])


def main(argv) -> int:
    from sim_a_splat_amd.rasterizer import Rasterizer
    n_seeds = int(argv[1]) if len(argv) > 1 else 60
    first = int(argv[2]) if len(argv) > 2 else 0
    poison_all = len(argv) > 3 and argv[3] == "poison-all"
    r = Rasterizer(0)
    bad, arms = 0, dict.fromkeys(ARMS, 0)
    for seed in range(first, first + n_seeds):
        c = draw_case(seed, poison_all)
        diffs = run_case(r, c)
        arms[c["arm"]] += 1
        print(describe(c), "->", "equal" if not diffs else "DIFFERENT: " + "; ".join(diffs), flush=True)
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
    print(f"{n_seeds} {'poisoned ' if poison_all else ''}cases from seed {first} (" + ", ".join(f"{a} {k}" for a, k in arms.items()) + "): " +
          ("every output equal to its reference" if bad == 0 else f"{bad} cases differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
