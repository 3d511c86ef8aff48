"""The scenes and cameras the feature and mesh tests share, their oracle frame, and what the GPU tests do with a Rasterizer: upload a
scene, fetch a frame, compare two frames bit for bit.  A scene is a dict of arrays (means, op, colors, sh, quats, scales, cov6, gid,
G, Rt); a camera is (V, K, W, H).  The fixtures are read with np.load here, not through conftest.py: fuzzers and probes import this
module outside pytest."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402
from sim_a_splat_amd.synthetic import (config_scene_and_cameras, intrinsics, look_at_viewmat, make_scene, random_group_poses,  # noqa: E402
                                       ring_camera)

GOLDEN = ROOT / "tests" / "golden"
OUTS = ("rgb", "alpha", "depth", "rgb8")


def twin(name):
    g = np.load(GOLDEN / f"render_twin_{name}.npz")
    kw = dict(quats=None, scales=None, cov6=None)
    if g["cov6"].size:
        kw["cov6"] = g["cov6"]
    else:
        kw.update(quats=g["quats"], scales=g["scales"])
    gid = g["group_id"] if g["group_id"].size else None
    W, H = [int(v) for v in g["wh"]]
    sc = dict(means=g["means"], op=g["opacities"], colors=g["colors"], sh=int(g["sh_degree"]), gid=gid,
              G=int(g["group_Rt"].shape[0]) if gid is not None else 0, Rt=g["group_Rt"] if gid is not None else None, **kw)
    return sc, (np.asarray(g["viewmat"], np.float32).reshape(4, 4), np.asarray(g["K"], np.float32).reshape(3, 3), W, H)


def synthetic(n, seed, ls, n_groups=0):
    s = make_scene(n, seed=seed, log_scale_mean=float(np.log(ls)), n_groups=n_groups)
    G = n_groups if s.group_id is not None else 0
    return dict(means=s.means, op=s.opacities, colors=s.sh, sh=s.sh_degree, quats=s.quats, scales=s.scales, cov6=None,
                gid=s.group_id, G=G, Rt=random_group_poses(G, seed + 1) if G else None)


def config3_window():
    s, cams = config_scene_and_cameras(3)
    cam = cams[0]
    K = np.array(cam.K, np.float32).copy()
    K[0, 2] -= 800.0      # a 320 x 240 window of the 1080p view, around its centre
    K[1, 2] -= 420.0
    sc = dict(means=s.means, op=s.opacities, colors=s.sh, sh=s.sh_degree, quats=s.quats, scales=s.scales, cov6=None,
              gid=None, G=0, Rt=None)
    return sc, (np.asarray(cam.viewmat, np.float32), K, 320, 240)


def ring(W=96, H=64, f=90.0, yaw=15.0, elev=0.2):
    c = ring_camera(W, H, f, yaw_deg=yaw, elev=elev)
    return np.asarray(c.viewmat, np.float32), np.asarray(c.K, np.float32), W, H


def general(W, H, fx, fy, cx, cy, eye, target=(0.0, 0.0, 0.0), roll_deg=0.0):
    """A pinhole camera with its own fx, fy and principal point, at ``eye`` looking at ``target``, rolled by ``roll_deg`` about its
    optical axis: V = Rz(roll) look_at(eye, target)."""
    a = np.deg2rad(roll_deg)
    Rz = np.eye(4)
    Rz[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    V = Rz @ np.asarray(look_at_viewmat(eye, target), np.float64)
    return V.astype(np.float32), np.asarray(intrinsics(fx, fy, cx, cy), np.float32), W, H


def oracle_frame(sc, cam, bg, keep=None, Rt=None, **kw):
    V, K, W, H = cam
    sel = slice(None) if keep is None else keep
    pick = lambda a: None if a is None else np.asarray(a)[sel]
    return oracle.render(pick(sc["means"]), pick(sc["op"]), pick(sc["colors"]), V, K, W, H, quats=pick(sc["quats"]),
                         scales=pick(sc["scales"]), cov6=pick(sc["cov6"]), sh_degree=sc["sh"], group_id=pick(sc["gid"]),
                         group_Rt=(sc["Rt"] if Rt is None else Rt) if sc["gid"] is not None else None, background=bg,
                         want_rgb8=True, **kw)


# ---- GPU side: what the tests do with a Rasterizer ------------------------------------------------------------------------
def upload(r, sc, keep=None, colors=None):
    """The scene, or (colors [n,3]) the same geometry recoloured with final RGB."""
    sel = slice(None) if keep is None else keep
    pick = lambda a: None if a is None else np.asarray(a)[sel]
    r.upload(pick(sc["means"]), pick(sc["op"]), pick(sc["colors"] if colors is None else colors), quats=pick(sc["quats"]),
             scales=pick(sc["scales"]), covariances=pick(sc["cov6"]), sh_degree=sc["sh"] if colors is None else -1,
             group_id=pick(sc["gid"]), n_groups=sc["G"])
    if sc["G"]:
        r.set_group_poses(sc["Rt"])


def to_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b, keys=OUTS, where=None):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if where is not None:
            x, y = x[where], y[where]
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (k, np.abs(x.astype(np.float64) - y).max())
