"""The adjoint of the deformation to the REST arrays under torch autograd ("Deformation": the adjoint to the rest arrays;
csrc/sas_skin.hip, k_deform_rest_grad), the cases the CPU and GPU tests of ``Rasterizer.deform_backward_rest`` share, and the recovery case
of ``deform.fit_dynamic_scene`` with its float64 stand-in renderer.  Every case is from a fixed seed.

``skin_grad_ref.deform_torch`` takes its rest arrays as arrays or as TENSORS, which it uses as they are: a gradient flows to them;
tests/test_skin_rest_cpu.py holds the two call forms to each other bit for bit, in float64 and in float32, on every case.
``rest_grad_ref`` is its vector-Jacobian product with respect to the rest tensors: float64 is the reference; float32 restates the device's
arithmetic up to the order of the sums over a Gaussian's entries, which autograd chooses: ``f32_err`` is the largest error, per array, of
the float32 evaluation against the float64 one over ORDERS shuffled orders of the entries (each order against the float64 evaluation in
that same order: a shuffle may change q_first, and with it the sign of q_b), and the GPU test's bound is four times that, in
``skin_ref.rel_err``.  ``skin_grad_ref.margins`` keeps every decision of every case MARGIN from its threshold, in every one of those orders.

    python tests/tools/skin_rest_ref.py      prints the F32_ERR table of tests/test_gpu_zf_skin_rest.py, the margins and, last, the recovery
                                             runs on the float64 reference (about a minute each)
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository: the recovery case runs deform.fit_dynamic_scene
import skin_grad_ref as sg  # noqa: E402
import skin_ref  # noqa: E402
from skin_grad_ref import deform_torch, node_quats_torch  # noqa: E402,F401

MARGIN = sg.MARGIN
ORDERS = 4              # shuffled entry orders of f32_err


def live_rows(indices, weights, m: int) -> np.ndarray:
    """[N] bool: the Gaussian has a live entry under ``m`` nodes."""
    idx, w = np.asarray(indices), np.asarray(weights)
    return ((idx >= 0) & (idx < m) & (w > 0)).any(axis=1)


def rest_grad_ref(rest, indices, weights, node_Rt, d_means=None, d_orient=None, dtype=torch.float64, order=None, bound_only=False) -> dict:
    """The gradient of ``sum(d_means * means') + sum(d_orient * orientation')`` with respect to the REST arrays, evaluated in ``dtype``: a dict
    of float64 arrays under ``means`` and the orientation key, for the upstream gradients given.  ``rest``: float32 arrays (they reach the
    restatement as float32 values, as they reach the device).  ``order``: a permutation of the k entry columns to evaluate them in.
    ``bound_only``: rows of Gaussians without a live entry are zero instead of the upstream gradient."""
    key = sg.orient_key(rest)
    idx, w = np.asarray(indices), np.asarray(weights, np.float32)
    if order is not None:
        idx, w = idx[:, np.asarray(order)], w[:, np.asarray(order)]
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(dtype).requires_grad_(True)
    P = {"means": leaf(rest["means"]), key: leaf(rest[key])}
    m = np.asarray(node_Rt).reshape(-1, 3, 4).shape[0]
    out = deform_torch(P, idx, w, torch.from_numpy(np.ascontiguousarray(np.asarray(node_Rt, np.float32).reshape(-1, 3, 4))), dtype)
    loss = torch.zeros((), dtype=dtype)
    given = []
    for k, d in (("means", d_means), (key, d_orient)):
        if d is not None:
            loss = loss + (out[k] * torch.from_numpy(np.asarray(d, np.float32)).to(dtype)).sum()
            given.append(k)
    loss.backward()
    keep = live_rows(idx, w, m) if bound_only else np.ones(idx.shape[0], bool)
    res = {}
    for k in given:
        g = np.zeros(tuple(P[k].shape)) if P[k].grad is None else P[k].grad.numpy().astype(np.float64)
        res[k] = np.where(keep[:, None], g, 0.0)
    return res


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
# name -> (Gaussians, node set, k, transforms' keyword arguments, bind's keyword arguments).  N = 1, 257 and 300: the last workgroup is partial;
# M = 9, 256 and 257: k_deform_rest_grad's LDS path, its last size and the global path; k = 1, 4, 5, 8: both KP instantiations.  The case at the
# LDS limit draws its transforms from seed 84: with the default (80) a shuffled entry order leaves it a dot of 1.0e-5, under MARGIN.
CASES = {
    "n1_m9_k1": (1, "m9", 1, dict(angle=3.1), {}),
    "n257_m9_k4": (257, "m9", 4, dict(angle=3.1), {}),
    "n300_m256_k5": (300, "m256", 5, dict(angle=3.1, seed=84), {}),          # the last size of the LDS path
    "n300_m257_k8": (300, "m257", 8, dict(angle=3.1), {}),          # ... and one past it: the global path
    "n300_m9_far": (300, "m9", 4, dict(angle=3.1), dict(max_distance=0.45)),   # Gaussians without a live entry
    "n300_m9_group": (300, "m9", 4, dict(angle=3.1), dict(group=1)),          # a group= bind
    "n300_m70_dead": (300, "m70", 4, dict(angle=3.1), dict(dead=True)),       # hand-set dead entries
}
FORMS = sg.FORMS


@functools.lru_cache(maxsize=None)
def case(name: str, form: str = "quats") -> dict:
    """One case, as ``skin_grad_ref.case`` makes its own: the scene, ``nodes``, the binding, ``bind``, ``transforms`` and the upstream
    gradients ``d_means`` and ``d_orient``.  Shared and never written."""
    n, node_set, k, tkw, bkw = CASES[name]
    kw = skin_ref.scene(form, n=n)
    q = skin_ref.nodes(node_set)
    m = q.shape[0]
    bind = {a: b for a, b in bkw.items() if a != "dead"}
    d2, index = skin_ref.knn_cross_ref(kw["means"], q, k, bind.get("max_distance", np.inf))
    keep = None if "group" not in bind else kw["group_id"] == bind["group"]
    idx, w = skin_ref.weights_ref(d2, index, skin_ref.default_sigma(q), np.float32, keep)
    if bkw.get("dead"):
        idx, w = sg.kill_entries(idx, w, m)
    rng = np.random.default_rng(1900 + 2 * list(CASES).index(name) + (form == "covariances"))   # every case and form its own draw
    return dict(name=name, form=form, scene=kw, rest=skin_ref.rest_of(kw), nodes=q, m=m, k=k, n=n, indices=idx.astype(np.int32),
                weights=w.astype(np.float32), bind=dict(k=k, **bind), dead=bool(bkw.get("dead")), transforms=skin_ref.transforms(q, **tkw),
                d_means=rng.normal(size=(n, 3)).astype(np.float32), d_orient=rng.normal(size=(n, 4 if form == "quats" else 6)).astype(np.float32))


def entry_orders(k: int):
    """The ORDERS fixed shuffled orders of k entry columns."""
    return [np.random.default_rng(7100 + s).permutation(k) for s in range(ORDERS)]


@functools.lru_cache(maxsize=None)
def grad64(name: str, form: str = "quats", means: bool = True, orient: bool = True, bound_only: bool = False) -> dict:
    """The reference of a case: ``rest_grad_ref`` in float64."""
    c = case(name, form)
    return rest_grad_ref(c["rest"], c["indices"], c["weights"], c["transforms"], c["d_means"] if means else None, c["d_orient"] if orient else None,
                         bound_only=bound_only)


def errs(got: dict, ref: dict) -> dict:
    """``skin_ref.rel_err`` per array."""
    return {k: skin_ref.rel_err(got[k], ref[k]) for k in ref}


def f32_err_of(rest, indices, weights, node_Rt, d_means, d_orient) -> dict:
    """The float32 restatement's own error against float64 per array: the largest over ORDERS shuffled entry orders, each against the float64
    evaluation in the same order."""
    worst = {}
    for order in entry_orders(np.asarray(indices).shape[1]):
        ref = rest_grad_ref(rest, indices, weights, node_Rt, d_means, d_orient, torch.float64, order)
        e = errs(rest_grad_ref(rest, indices, weights, node_Rt, d_means, d_orient, torch.float32, order), ref)
        worst = {k: max(worst.get(k, 0.0), v) for k, v in e.items()}
    return worst


def f32_err(name: str, form: str = "quats", means: bool = True, orient: bool = True) -> dict:
    c = case(name, form)
    return f32_err_of(c["rest"], c["indices"], c["weights"], c["transforms"], c["d_means"] if means else None, c["d_orient"] if orient else None)


def case_margins(name: str) -> dict:
    """``skin_grad_ref.margins`` of a case, the smallest over the entry orders of f32_err and the order as bound."""
    c = case(name)
    out = None
    for order in [np.arange(c["k"])] + entry_orders(c["k"]):
        mg = sg.margins(c["indices"][:, order], c["weights"][:, order], c["transforms"])
        out = mg if out is None else dict(out, dot=min(out["dot"], mg["dot"]), n2=min(out["n2"], mg["n2"]), flips=max(out["flips"], mg["flips"]))
    return out


# ---- the recovery case: the kit's sheet seen in two bends; its rest means perturbed and its colours tinted, fitted back -------------------------
DYN_ITERS = 30
# The noise on the rest means (scene units; the Gaussians are 0.035 to 0.06 wide): a smooth random field of this amplitude per axis -- three
# plane waves across the sheet -- plus white noise.  White noise alone is not what this sheet's pictures determine: most of its Gaussians lie
# under their neighbours (300 of them, opacity 0.6 to 0.95, on 1.0 x 0.8), and with sigma 0.02 per axis the reference run ends at 0.947 of its
# start after 30 iterations and at 0.924 after 60, while the loss falls to a fifth.  Noise that neighbours share moves what the cameras see.
DYN_NOISE = 0.03
DYN_WHITE = 0.004
DYN_TINT = (0.25, -0.2, 0.15)
DYN_LRS = dict(means=4e-3, sh_dc=2e-1)
DYN_BEND_B = -0.05         # the second bend: the rim along y sinks, z += DYN_BEND_B (2.5 y)^2
# where the float64 reference runs end: the rest means' mean distance to the truth as a fraction of its start, transforms known / the second
# bend's fitted from the identity (tests/test_skin_rest_cpu.py holds the runs to them; the GPU runs are compared with them)
DYN_REF_END = 0.8572
DYN_JOINT_REF_END = 0.8629
# No case of this size comes near the truth: the sheet's pictures do not determine the Gaussians that lie under others.  As with
# skin_grad_ref.RECOVER_FRACTION, the ratio reached, rounded up to one digit, stands in.
DYN_FRACTION = 0.9
DYN_JOINT_FRACTION = 0.9
# The joint run does not find the second bend at this size: the largest entry of its transforms' error goes from 0.0543 (the identity) to 0.0523
# in 30 iterations -- the rest means take the pictures' error up faster than the nodes do.  So the joint mode is held by its whole loss history
# too, every iteration within 0.05 of the start loss of the reference's:
DYN_JOINT_HISTORY = (0.017493, 0.012056, 0.009577, 0.009716, 0.009347, 0.007421, 0.005849, 0.006422, 0.006698, 0.005939, 0.004846, 0.004672,
                     0.004975, 0.004808, 0.00426, 0.004002, 0.004044, 0.00396, 0.003723, 0.003573, 0.003552, 0.003473, 0.0033, 0.00322, 0.003226,
                     0.00312, 0.003021, 0.00297, 0.002939, 0.002889)


@functools.lru_cache(maxsize=None)
def dynamic_case() -> dict:
    """``skin_grad_ref.recovery_case``'s sheet, nodes, binding and cameras; two bends (the kit's trough along x, and a ridge along y) as known
    node transforms; ``frames``: the float64 reference's frames of the TRUE sheet in each bend, as ``fit_dynamic_scene`` takes them;
    ``start``: the scene to upload, its means perturbed and its colours tinted."""
    from sim_a_splat_amd import deform
    c = dict(sg.recovery_case())
    nodes = c["nodes"]
    moved = nodes.astype(np.float64)
    moved[:, 2] += DYN_BEND_B * (2.5 * moved[:, 1]) ** 2
    bends = np.stack([c["truth"], deform.transforms_from_positions(nodes, moved).astype(np.float64)])
    V, K = np.stack([cam[0] for cam in c["cams"]]), np.stack([cam[1] for cam in c["cams"]])
    true = DynRefRenderer(c, c["upload"])
    frames = []
    with torch.no_grad():
        for T in bends:
            true.deform(T.astype(np.float32))
            frames.append(dict(images=np.stack([true.render(V[v], K[v], sg.RECOVER_W, sg.RECOVER_H)["rgb"].numpy() for v in range(len(V))]).astype(np.float32),
                               viewmats=V, Ks=K))
    rng = np.random.default_rng(5152)
    n = sg.RECOVER_N
    m = c["upload"]["means"].astype(np.float64)
    d = np.zeros_like(m)
    for axis in range(3):
        for _ in range(3):
            wave = rng.normal(0.0, 4.0, 3)
            wave[2] = 0.0
            d[:, axis] += np.sin(m @ wave + rng.uniform(0.0, 6.28))
    d = d * (DYN_NOISE / np.sqrt(1.5)) + rng.normal(0.0, DYN_WHITE, m.shape)
    start = dict(c["upload"], means=(m + d).astype(np.float32),
                 colors=np.clip(c["upload"]["colors"] * np.float32(0.7) + np.asarray(DYN_TINT, np.float32), 0.02, 0.98).astype(np.float32))
    c.update(bends=bends, frames=frames, start=start, V=V, K=K)
    return c


class DynRefRenderer:
    """The rasterizer's methods ``fit_dynamic_scene`` uses, on the float64 references: ``deform_torch`` bends, grad_ref renders and
    differentiates, ``rest_grad_ref``'s function and ``skin_grad_ref``'s are the adjoints, fit_ref steps.  The state is the REST scene."""
    covariance_form = "quats"
    has_skin = True

    def __init__(self, c, upload):
        import fit_ref
        n = np.asarray(upload["means"]).shape[0]
        self.c = c
        self.S = fit_ref.new_state(dict(means=upload["means"], opacities=upload["opacities"], colors=np.asarray(upload["colors"]).reshape(n, 1, 3),
                                        quats=upload["quats"], scales=upload["scales"]), np.float64)
        self.T = None
        self._last = None

    def read_skin(self):
        return dict(indices=torch.from_numpy(self.c["indices"]), weights=torch.from_numpy(self.c["weights"]))

    def deform(self, T):
        self.T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(-1, 3, 4))

    def clear_skin(self):
        self.T = None

    def _bend(self, P):
        """The deformed means and quats (tensors) of rest tensors ``P`` under the current transforms."""
        if self.T is None:
            return dict(means=P["means"], quats=P["quats"])
        return deform_torch(P, self.c["indices"], self.c["weights"], torch.from_numpy(self.T.astype(np.float64)), torch.float64)

    def read_scene(self):
        x = self.S["x"]
        with torch.no_grad():
            bent = self._bend(dict(means=torch.from_numpy(x["means"]), quats=torch.from_numpy(x["quats"])))
        return dict({k: torch.tensor(v) for k, v in x.items()}, means=bent["means"].clone(), quats=bent["quats"].clone())

    def render(self, V, K, W, H, background=(0.0, 0.0, 0.0), **kw):
        import grad_ref
        x = self.read_scene()
        sc = dict(means=x["means"].numpy(), op=x["opacities"].numpy(), colors=x["colors"].numpy(), sh=-1, quats=x["quats"].numpy(),
                  scales=x["scales"].numpy(), cov6=None, gid=None, G=0, Rt=None)
        P, vm, I, F = grad_ref.forward(sc, (V, K, W, H))
        self._last = (np.asarray(V).tobytes(), P, F)
        out = grad_ref.finish({k: v.detach() for k, v in F.items() if k != "near"}, background)
        return dict(rgb=out["rgb"], alpha=out["alpha"][..., None], depth=out["depth"][..., None])

    def render_backward(self, V, K, W, H, g_rgb=None, g_alpha=None, g_depth=None, *, out=None, want=None, **kw):
        """Gradients of the DEFORMED arrays, as the device returns them on a skinned scene."""
        if self._last is None or self._last[0] != np.asarray(V).tobytes():
            self.render(V, K, W, H)
        _, P, F = self._last
        self._last = None
        loss = sum((g.double().reshape(f.shape) * f).sum() for g, f in ((g_rgb, F["acc_rgb"]), (g_alpha, F["alpha"]), (g_depth, F["acc_z"])) if g is not None)
        loss.backward()
        names = dict(means="means", opacities="op", colors="colors", quats="quats", scales="scales")
        res = dict(out or {})
        for k in (want or names):
            g = P[names[k]].grad
            g = torch.zeros_like(P[names[k]]) if g is None else g
            res[k] = g.detach().clone() if res.get(k) is None else res[k] + g.detach()
        return res

    def deform_backward_rest(self, grads, out=None, bound_only=False):
        x = self.S["x"]
        P = {k: torch.from_numpy(x[k]).clone().requires_grad_(True) for k in ("means", "quats")}
        bent = self._bend(P)
        sum((bent[k] * grads[k].double()).sum() for k in grads).backward()
        keep = torch.from_numpy(live_rows(self.c["indices"], self.c["weights"], self.T.shape[0]) if bound_only else np.ones(self.S["n"], bool))
        res = dict(out or {})
        for k in grads:
            g = torch.where(keep[:, None], P[k].grad, torch.zeros_like(P[k].grad))
            res[k] = g.clone() if res.get(k) is None else res[k] + g
        return res

    def deform_backward(self, grads):
        x = self.S["x"]
        rest = dict(means=torch.from_numpy(x["means"]), quats=torch.from_numpy(x["quats"]))
        G = torch.from_numpy(self.T.astype(np.float64)).requires_grad_(True)
        bent = deform_torch(rest, self.c["indices"], self.c["weights"], G, torch.float64)
        sum((bent[k] * grads[k].double()).sum() for k in ("means", "quats") if grads.get(k) is not None).backward()
        return G.grad

    def adam_reset(self):
        for k in ("m", "v", "raw"):
            self.S[k].clear()

    def adam_step(self, grads, lrs, step, betas=(0.9, 0.999), eps=1e-15, visible_only=False, rest=False):
        import fit_ref
        assert rest, "the state is the rest scene"
        fit_ref.step(self.S, {k: v.numpy() for k, v in grads.items()}, lrs, step, betas, eps, visible_only)


def rest_error(c, means) -> float:
    """The mean distance of rest means to the case's true rest means."""
    return float(np.linalg.norm(np.asarray(means, np.float64) - c["upload"]["means"].astype(np.float64), axis=1).mean())


def dynamic_settings(joint: bool = False) -> dict:
    """``fit_dynamic_scene``'s keyword arguments of the recovery runs: transforms known, or (``joint``) the second bend's started at the identity."""
    c = dynamic_case()
    T = c["bends"].copy()
    if joint:
        T[1] = skin_ref.identity_transforms(9)
    return dict(what=("means", "colors"), transforms=T, fit_transforms=joint, iters=DYN_ITERS, lrs=DYN_LRS, extent=1.0)


def recover_on_reference(joint: bool = False):
    """The recovery case run on the float64 reference: (DynamicFit, start error, end error, the stand-in)."""
    from sim_a_splat_amd import deform
    c = dynamic_case()
    R = DynRefRenderer(c, c["start"])
    res = deform.fit_dynamic_scene(None, c["frames"], c["nodes"], renderer=R, **dynamic_settings(joint))
    R.clear_skin()
    return res, rest_error(c, c["start"]["means"]), rest_error(c, R.read_scene()["means"].numpy()), R


if __name__ == "__main__":
    print("F32_ERR = {   # (case, form): per array, float32 restatement against float64, the largest of %d shuffled entry orders" % ORDERS)
    for name in CASES:
        for form in FORMS:
            e = f32_err(name, form)
            print(f'    ("{name}", "{form}"): dict(' + ", ".join(f"{k}={v:.2e}" for k, v in e.items()) + "),")
    print("}")
    for name in CASES:
        mg = case_margins(name)
        c = case(name)
        print(f"# {name}: branch margin {mg['branch']:.1e}, min |dot| {mg['dot']:.1e}, min n2 {mg['n2']:.1e}, branches {mg['branches']}, flips {mg['flips']}, "
              f"Gaussians without a live entry {int((~live_rows(c['indices'], c['weights'], c['m'])).sum())}")
    import time
    for joint in (False, True):
        t0 = time.time()
        res, e0, e1, _ = recover_on_reference(joint)
        print(f"# recovery, {'joint' if joint else 'transforms known'}: rest means' mean distance {e0:.5f} -> {e1:.5f} = {e1 / e0:.4f} of the start; "
              f"loss {res.history[0]:.4e} -> {res.history[-1]:.4e}; {time.time() - t0:.1f} s")
