"""CPU: the yardstick of density control (tests/tools/densify_ref.py), what the GPU tests assume of their cases
(tests/tools/densify_cases.py), and the schedule of fit.fit_scene(densify=) on a recording stand-in renderer.

- densify_ref against a plain per-Gaussian Python loop on the smallest mixed case,
- the generator: mean and variance of 24 576 normals, the two children of a parent differ,
- the float32 error table the GPU bounds rest on is current,
- the schedule fires at the right steps, the gradient buffers and statistics are made anew at the new N, n_history is right, and
  densify=None runs the calls it always ran,
- the new entry points are declared, bound and built; Python refuses bad configurations."""
import ctypes
import math
import struct
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, build, fit

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import densify_cases as dc  # noqa: E402
import densify_ref  # noqa: E402


def test_symbols_declared_listed_and_built():
    header = (Path(build.PKG).parent / "include" / "sim_a_splat_amd.h").read_text()
    L = _capi.lib()
    for name in ("sas_density_accumulate", "sas_scene_densify", "sas_scene_reset_opacity"):
        assert name in _capi.EXPORTS and f"int {name}(" in header and hasattr(L, name)
    assert build.CSRC / "sas_density.hip" in build.SOURCES
    assert "typedef struct sas_densify_config" in header
    for k, v in (("GROW", 1), ("PRUNE_OPACITY", 2), ("PRUNE_SCALE", 4)):
        assert f"#define SAS_DENSIFY_{k} {v}u" in header and getattr(_capi, f"SAS_DENSIFY_{k}") == v
    assert ctypes.sizeof(_capi.DensifyConfig) == 40 and _capi.DensifyConfig.max_gaussians.offset == 24
    assert len(L.sas_density_accumulate.argtypes) == 8 and len(L.sas_scene_densify.argtypes) == 7 and len(L.sas_scene_reset_opacity.argtypes) == 3
    for text in ("README.md", "sim_a_splat_amd/fit.py", "include/sim_a_splat_amd.h"):   # no longer out of scope
        assert "N is fixed" not in (Path(build.PKG).parent / text).read_text(), text


# ---- an independent restatement: one Gaussian at a time, Python integers and math ---------------------------------------------------
def _mix(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _normal(seed, parent, child, axis):
    base = _mix((_mix((seed & 0xffffffff) ^ 0x9e3779b9) + parent) & 0xffffffff)
    c = 2 * (3 * child + axis)
    h1, h2 = _mix(base ^ (((c + 1) * 0x9e3779b9) & 0xffffffff)), _mix(base ^ (((c + 2) * 0x9e3779b9) & 0xffffffff))
    u1, u2 = ((h1 >> 8) + 1) / 2.0 ** 24, (h2 >> 8) / 2.0 ** 24
    two_pi = struct.unpack("f", struct.pack("f", 6.2831855))[0]
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(two_pi * u2)


def _loop(sc, stats, cfg):
    f = np.float32
    n = sc["means"].shape[0]
    grow_scale, prune_scale = f(cfg["grow_scale3d"]) * f(cfg["scene_extent"]), f(cfg["prune_scale3d"]) * f(cfg["scene_extent"])
    cls = []
    for i in range(n):
        cnt = int(stats["count"][i])
        avg = f(stats["grad_sum"][i]) / f(max(cnt, 1))
        smax = max(sc["scales"][i])
        high = cnt > 0 and avg > f(cfg["grow_grad2d"])
        small = smax <= grow_scale
        pruned = sc["opacities"][i] < f(cfg["prune_opacity"]) or (smax > prune_scale and not (high and not small))
        cls.append("pruned" if pruned else "clone" if high and small else "split" if high else "stay")
    cap = cfg.get("max_gaussians", 0)
    room = (cap - sum(c != "pruned" for c in cls)) if cap > 0 else n
    for want in ("clone", "split"):   # the budget goes to the clones first, each class in index order
        for i in range(n):
            if cls[i] == want:
                if room <= 0:
                    cls[i] = "stay"
                room -= 1
    rows = [(i, None) for i in range(n) if cls[i] in ("stay", "clone")] + [(i, None) for i in range(n) if cls[i] == "clone"]
    rows += [(i, ch) for i in range(n) if cls[i] == "split" for ch in (0, 1)]
    means, scales = [], []
    for i, ch in rows:
        m, s = [float(v) for v in sc["means"][i]], sc["scales"][i]
        if ch is not None:
            w, x, y, z = (float(v) for v in sc["quats"][i])
            norm = math.sqrt(w * w + x * x + y * y + z * z)
            w, x, y, z = w / norm, x / norm, y / norm, z / norm
            R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
            d = [float(s[k]) * _normal(cfg["seed"], i, ch, k) for k in range(3)]
            m = [m[a] + sum(R[a][k] * d[k] for k in range(3)) for a in range(3)]
            s = s / f(cfg["split_factor"])
        means.append(m)
        scales.append(s)
    return [i for i, _ in rows], np.array(means), np.array(scales, np.float32), cls


@pytest.mark.parametrize("name", ["n63_sh3_groups", "n1"])
def test_restatement_against_a_plain_loop(name):
    sc, stats, cfg = dc.case(name)
    old, ref = dc.ref_scene(sc), dc.reference(name)
    parents, means, scales, cls = _loop(old, stats, cfg)
    assert parents == list(ref["parents"]) and len(parents) == ref["n"]
    assert (cls.count("clone"), cls.count("split"), cls.count("pruned")) == (ref["cloned"], ref["split"], ref["pruned"])
    assert np.abs(means - ref["scene"]["means"]).max() <= 1e-13
    assert np.array_equal(scales.view(np.uint32), np.ascontiguousarray(ref["scene"]["scales"]).view(np.uint32))
    for k in ("opacities", "colors", "quats", "gid"):
        if old[k] is not None:
            assert np.array_equal(ref["scene"][k], old[k][parents]), k


def test_the_cap_cuts_clones_first_then_splits():
    for name, cut in (("cap_clones", "clones"), ("cap_splits", "splits")):
        sc, stats, cfg = dc.case(name)
        ref = dc.reference(name)
        free = densify_ref.densify(dc.ref_scene(sc), stats, dict(cfg, max_gaussians=0))
        assert ref["n"] == cfg["max_gaussians"] < free["n"] and ref["pruned"] == free["pruned"]
        if cut == "clones":
            assert 0 < ref["cloned"] < free["cloned"] and ref["split"] == 0 < free["split"]
        else:
            assert ref["cloned"] == free["cloned"] and 0 < ref["split"] < free["split"]
        parents, _, _, cls = _loop(dc.ref_scene(sc), stats, cfg)
        assert parents == list(ref["parents"])
    assert dc.reference("nothing")["n"] == 600 and np.array_equal(dc.reference("nothing")["parents"], np.arange(600))
    assert dc.reference("all_split")["split"] == 600 and dc.reference("all_but_one_pruned")["n"] == 1
    big = dc.reference("big")
    assert dc.BIG == 256 * 257 + 3 and abs(big["cloned"] / dc.BIG - 0.3) < 0.02 and abs(big["split"] / dc.BIG - 0.3) < 0.02 and abs(big["pruned"] / dc.BIG - 0.2) < 0.02


def test_generator_statistics():
    """24 576 normals of 4 096 parents: a broken generator would be shared by the kernel and its restatement, so it is held to what
    standard normals give (five standard errors)."""
    z = densify_ref.normals(7, np.arange(4096))
    n = z.size
    assert z.shape == (4096, 2, 3) and n == 24576
    assert abs(z.mean()) <= 5.0 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert not np.any(np.all(z[:, 0] == z[:, 1], axis=1))
    assert len(np.unique(z)) > 0.999 * n and not np.array_equal(z, densify_ref.normals(8, np.arange(4096)))
    assert abs(z[5, 1, 2] - _normal(7, 5, 1, 2)) <= 1e-15
    u1, u2 = densify_ref.uniforms(7, np.arange(4096))
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    z32 = densify_ref.normals(7, np.arange(4096), np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-5


def test_float32_error_table_is_current():
    """densify_cases.F32_ERR (the GPU bound is four times it) is what densify_ref computes today: the cases that split, every figure
    within 5 %."""
    now = {name: dc.float32_error(name) for name in dc.NAMES}
    assert set(dc.F32_ERR) == {k for k, v in now.items() if v is not None}
    for k, v in dc.F32_ERR.items():
        assert now[k] > 0 and abs(v - now[k]) <= 0.05 * now[k], (k, v, now[k])


def test_accumulate_restatement():
    stats = dict(grad_sum=np.zeros(3, np.float32), count=np.zeros(3, np.int32), max_radius=np.zeros(3, np.float32))
    d = np.array([[3e-3, 4e-3], [1.0, 1.0], [0.0, 2e-3]], np.float32)
    densify_ref.accumulate(stats, d, np.array([[2, 5], [0, 0], [7, 1]]), 64, 48)
    densify_ref.accumulate(stats, d, np.array([[1, 1], [0, 0], [0, 0]]), 64, 48)
    want = math.hypot(32 * float(d[0, 0]), 24 * float(d[0, 1]))
    assert list(stats["count"]) == [2, 0, 1] and list(stats["max_radius"]) == [5.0, 0.0, 7.0]
    assert abs(stats["grad_sum"][0] - 2 * want) < 1e-7 and stats["grad_sum"][1] == 0 and abs(stats["grad_sum"][2] - 24 * 2e-3) < 1e-8


# ---- the schedule of fit_scene on a recording stand-in -------------------------------------------------------------------------------
class Recorder:
    """The methods fit_scene uses, on no scene at all: frames are zeros, a densify call adds ``grow`` Gaussians; every call is recorded."""

    def __init__(self, n, grow=0):
        self.n, self.grow, self.calls = n, grow, []

    def read_scene(self):
        return dict(means=torch.zeros(self.n, 3, dtype=torch.float64))

    def render(self, V, K, W, H, background=(0.0, 0.0, 0.0), **kw):
        self.calls.append(("render", np.asarray(V).tobytes()))
        return dict(rgb=torch.full((H, W, 3), 0.25, dtype=torch.float64), alpha=torch.zeros(H, W, 1, dtype=torch.float64), depth=torch.zeros(H, W, 1, dtype=torch.float64))

    def render_backward(self, V, K, W, H, g_rgb=None, g_alpha=None, g_depth=None, *, out=None, want=None, **kw):
        self.calls.append(("render_backward", np.asarray(V).tobytes(), None if out is None else int(out["colors"].shape[0])))
        res = dict(out or {})
        for k in want:
            if res.get(k) is None:
                res[k] = torch.zeros(self.n, 3)
        return res

    def adam_step(self, grads, lrs, step, **kw):
        self.calls.append(("adam_step", step, tuple(sorted(lrs)), {k: int(v.shape[0]) for k, v in grads.items()}))

    def new_density_stats(self):
        return dict(grad_sum=torch.zeros(self.n), count=torch.zeros(self.n, dtype=torch.int32), max_radius=torch.zeros(self.n))

    def density_accumulate(self, W, H, stats, d_means2d=None):
        stats["count"] += 1
        self.calls.append(("density_accumulate", W, H, int(stats["count"].shape[0]), int(stats["count"][0])))

    def densify(self, stats, **cfg):
        self.calls.append(("densify", int(stats["count"].shape[0]), int(stats["count"][0]), cfg))
        self.n += self.grow
        return dict(n=self.n)

    def reset_opacity(self, max_opacity=0.01):
        self.calls.append(("reset_opacity", max_opacity))


def _run(densify, grow=0, iters=12):
    rng = np.random.default_rng(1)
    V, K = rng.normal(size=(3, 4, 4)).astype(np.float32), rng.normal(size=(3, 3, 3)).astype(np.float32)
    R = Recorder(10, grow)
    res = fit.fit_scene(None, V, K, 4, 2, np.zeros((3, 2, 4, 3), np.float32), iters, what=("colors", "means"), views_per_step=2, renderer=R,
                        densify=densify, extent=2.5)
    return R, res


def test_fit_scene_schedule_on_a_recording_stand_in():
    cfg = fit.DensifyConfig(start=4, stop=11, every=2, reset_every=5, max_gaussians=99, seed=3)
    R, res = _run(cfg, grow=7)
    names = [c[0] for c in R.calls]
    step_at = lambda k: [c for c in R.calls[:k] if c[0] == "adam_step"][-1][1]   # the step a post-step call follows
    dens = [k for k, c in enumerate(R.calls) if c[0] == "densify"]
    assert [step_at(k) for k in dens] == [4, 6, 8, 10]                       # start <= t < stop, every second step
    assert [step_at(k) for k, c in enumerate(R.calls) if c[0] == "reset_opacity"] == [5, 10]
    assert all(names[k - 1] == "adam_step" for k in dens) and names[dens[-1] + 1] == "reset_opacity"   # densify first, then the reset
    # every backward pass is followed by its accumulate; the statistics count the views since the last densify
    for k, c in enumerate(R.calls):
        if c[0] == "render_backward":
            assert names[k + 1] == "density_accumulate" and R.calls[k + 1][1:3] == (4, 2)
    assert [R.calls[k][1:3] for k in dens] == [(10, 8), (17, 4), (24, 4), (31, 4)]   # (N of the statistics, views accumulated)
    # the configuration reaches densify; scales are pruned only once a reset has happened
    sent = [R.calls[k][3] for k in dens]
    assert [s["prune_scale_on"] for s in sent] == [False, True, True, True] and [s["seed"] for s in sent] == [7, 9, 11, 13]
    assert all(s["scene_extent"] == 2.5 and s["max_gaussians"] == 99 and s["grow_grad2d"] == 2e-4 and s["split_factor"] == 1.6 for s in sent)
    assert [c[1] for c in R.calls if c[0] == "reset_opacity"] == [0.01, 0.01]
    # the gradient buffers are made anew at the new N: the first backward pass of a step gets none, the second the first's
    sizes = {c[1]: c[3] for c in R.calls if c[0] == "adam_step"}
    assert [sizes[t]["colors"] for t in range(1, 13)] == [10] * 4 + [17] * 2 + [24] * 2 + [31] * 2 + [38] * 2
    firsts = [c[2] for c in R.calls if c[0] == "render_backward"][0::2]
    assert firsts == [None] * 12
    assert res.n_history == [10] * 3 + [17] * 2 + [24] * 2 + [31] * 2 + [38] * 3 and res.steps == 12


def test_without_densify_the_loop_is_the_one_it_was():
    plain, res0 = _run(None)
    never, res1 = _run(fit.DensifyConfig(start=100, every=100, reset_every=0))
    assert res0.n_history == [] and res1.n_history == [10] * 12 and res0.history == res1.history and len(res0.history) == 12
    assert {c[0] for c in plain.calls} == {"render", "render_backward", "adam_step"}
    assert [c for c in never.calls if c[0] != "density_accumulate"] == plain.calls
    assert sum(c[0] == "density_accumulate" for c in never.calls) == 24
    # the sequence of the loop before density control: per step, (render, render_backward) per view, then the step
    assert [c[0] for c in plain.calls] == ["render", "render_backward", "render", "render_backward", "adam_step"] * 12


def test_validation_in_python():
    for bad in (dict(every=0), dict(start=-1), dict(grow_grad2d=-1.0), dict(prune_opacity=float("nan")), dict(split_factor=1.0), dict(max_gaussians=-1),
                dict(reset_opacity=1.0)):
        with pytest.raises(ValueError, match="DensifyConfig"):
            _run(fit.DensifyConfig(**bad))

    class NoDensity(Recorder):
        pass
    NoDensity.densify = property(lambda self: (_ for _ in ()).throw(AttributeError()))
    with pytest.raises(ValueError, match="needs a renderer with"):
        rng = np.random.default_rng(1)
        fit.fit_scene(None, rng.normal(size=(1, 4, 4)), rng.normal(size=(1, 3, 3)), 4, 2, np.zeros((1, 2, 4, 3), np.float32), 2, renderer=NoDensity(3),
                      densify=fit.DensifyConfig())
    d = fit.DensifyConfig()
    assert (d.start, d.stop, d.every, d.reset_every, d.grow_grad2d, d.grow_scale3d, d.prune_opacity, d.prune_scale3d, d.max_gaussians, d.seed) == \
        (500, 15000, 100, 3000, 2e-4, 0.01, 0.005, 0.1, 0, 0)
