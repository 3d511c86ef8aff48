"""CPU: the yardstick of MCMC density control (tests/tools/mcmc_ref.py), what the GPU tests assume of their cases
(tests/tools/mcmc_cases.py), and the schedule of fit.fit_scene(densify=McmcConfig) on a recording stand-in renderer.

- the new entry points are declared, bound and built; the config struct's layout,
- mcmc_ref against a plain per-Gaussian, per-draw Python loop (integers and math) on the smallest mixed case,
- sampled frequencies follow the opacities; the n_grow arithmetic at the cap's edges; the dominated case has its many copies,
- the float32 error tables the GPU bounds rest on are current,
- the schedule: refine at the right steps, noise every step at the decayed rate times noise_lr, the regularisers' constants at the current
  N, n_history; densify=None and a DensifyConfig run the calls they always ran; Python refuses bad configurations."""
import ctypes
import math
import struct
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, build, fit
from sim_a_splat_amd.rasterizer import Rasterizer

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mcmc_cases as mc  # noqa: E402
import mcmc_ref  # noqa: E402


def test_symbols_declared_listed_and_built():
    header = (Path(build.PKG).parent / "include" / "sim_a_splat_amd.h").read_text()
    L = _capi.lib()
    for name in ("sas_scene_mcmc_noise", "sas_scene_mcmc_refine"):
        assert name in _capi.EXPORTS and f"int {name}(" in header and hasattr(L, name)
    assert build.CSRC / "sas_mcmc.hip" in build.SOURCES
    assert "typedef struct sas_mcmc_config" in header
    C = _capi.McmcConfig
    assert ctypes.sizeof(C) == 24 and (C.cap_max.offset, C.grow_factor.offset, C.min_opacity.offset, C.seed.offset) == (0, 8, 16, 20)
    assert len(L.sas_scene_mcmc_noise.argtypes) == 5 and len(L.sas_scene_mcmc_refine.argtypes) == 5
    assert hasattr(Rasterizer, "mcmc_noise") and hasattr(Rasterizer, "mcmc_refine")


# ---- an independent restatement: one Gaussian and one draw at a time, Python integers and math ---------------------------------------
def _mix(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _loop_refine(op, scales, cfg):
    n = len(op)
    thr = _f32(cfg["min_opacity"])
    alive = [float(o) > thr for o in op]
    w = [int(_f32(float(o) * 16777216.0)) if a else 0 for o, a in zip(op, alive)]
    prefix, run = [], 0
    for x in w:
        run += x
        prefix.append(run)
    n_alive = sum(alive)
    n_grow = max(0, min(cfg["cap_max"], int(math.floor(cfg["grow_factor"] * n))) - n)
    draws = n - n_alive + n_grow
    src, copies = [], [0] * n
    for d in range(draws):
        base = _mix((_mix((cfg["seed"] & 0xffffffff) ^ 0x9e3779b9) + d) & 0xffffffff)
        u = (_mix(base ^ 0x9e3779b9) << 32) | _mix(base ^ ((2 * 0x9e3779b9) & 0xffffffff))
        t = (u * run) >> 64
        i = next(k for k in range(n) if (prefix[k - 1] if k else 0) <= t < prefix[k])
        src.append(i)
        copies[i] += 1
    parents = [i for i in range(n) if alive[i]] + src
    new_o, new_s = {}, {}
    for i in range(n):
        if copies[i] == 0:
            continue
        m = min(copies[i] + 1, 51)
        o = float(op[i])
        on = 1.0 - math.pow(1.0 - o, 1.0 / m)
        denom = 0.0
        for a in range(1, m + 1):
            for k in range(a):
                denom += (float(math.comb(a - 1, k)) * ((-1.0) ** k * on ** (k + 1))) / math.sqrt(k + 1)
        new_o[i] = min(max(_f32(on), thr), _f32(1.0 - 2.0 ** -23))
        new_s[i] = [_f32(_f32(o / denom) * float(s)) for s in scales[i]]
    return parents, copies, n - n_alive, n_grow, new_o, new_s


def test_restatement_against_a_plain_loop():
    name = "n63_sh3_groups"
    sc, cfg = mc.case(name)
    ref = mc.reference(name)
    parents, copies, n_dead, n_grow, new_o, new_s = _loop_refine(sc["op"], sc["scales"], cfg)
    assert n_dead > 10 and n_grow == 3 and max(copies) >= 3
    assert (ref["n"], ref["relocated"], ref["added"]) == (len(parents), n_dead, n_grow) and ref["n"] == 63 + n_grow
    assert np.array_equal(ref["parents"], parents) and np.array_equal(ref["copies"], copies)
    got = ref["scene"]
    for pos, i in enumerate(parents):
        if copies[i]:
            assert ref["fresh"][pos]
            assert abs(float(got["opacities"][pos]) - new_o[i]) <= float(np.spacing(np.float32(new_o[i])))
            assert np.all(np.abs(got["scales"][pos].astype(np.float64) - new_s[i]) <= np.spacing(np.asarray(new_s[i], np.float32)))
        else:
            assert not ref["fresh"][pos] and got["opacities"][pos] == sc["op"][i] and np.array_equal(got["scales"][pos], sc["scales"][i])
        assert np.array_equal(got["means"][pos], sc["means"][i]) and np.array_equal(got["quats"][pos], sc["quats"][i])
        assert np.array_equal(got["colors"][pos], sc["colors"][i]) and got["gid"][pos] == sc["gid"][i]


def test_sampled_frequencies_follow_the_opacities():
    op = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    alive, w = mcmc_ref.decide(op, 0.005)
    D = 40000
    src, copies = mcmc_ref.sample(w, D, seed=17)
    assert alive.all() and copies.sum() == D and len(src) == D
    p = w.astype(np.float64) / float(w.sum())
    sd = np.sqrt(D * p * (1.0 - p))
    assert np.all(np.abs(copies - D * p) <= 5.0 * sd), (copies, D * p, sd)
    # a dead Gaussian is never drawn, wherever it stands; a NaN opacity is dead
    alive, w = mcmc_ref.decide(np.array([0.001, 0.5, np.nan, 0.5, 0.0], np.float32), 0.005)
    assert alive.tolist() == [False, True, False, True, False]
    assert mcmc_ref.sample(w, 1000, seed=1)[1][[0, 2, 4]].tolist() == [0, 0, 0]


def test_grow_count_at_the_caps_edges():
    g = mcmc_ref.grow_count
    assert g(600, 10 ** 6, 1.05) == 30 and g(600, 600, 1.05) == 0 and g(600, 599, 1.05) == 0 and g(600, 601, 1.05) == 1 and g(600, 630, 1.05) == 30
    assert g(600, 629, 1.05) == 29 and g(1, 10 ** 6, 1.05) == 0 and g(19, 10 ** 6, 1.05) == 0 and g(20, 10 ** 6, 1.05) == 1
    assert g(600, 10 ** 6, 1.0) == 0 and g(1, 10 ** 6, 2.0) == 1 and g(mc.BIG, 10 ** 6, 1.05) == int(math.floor(1.05 * mc.BIG)) - mc.BIG
    for name in mc.NAMES:   # N_new = N + n_grow always; what the kinds promise
        n, r = mc.CASES[name][0], mc.reference(name)
        assert r["n"] == n + r["added"] == len(r["parents"]) and r["n"] <= max(n, mc.case(name)[1]["cap_max"])
    assert mc.reference("relocate_only")["added"] == 0 and mc.reference("relocate_only")["relocated"] > 100
    assert mc.reference("grow_only")["relocated"] == 0 and mc.reference("grow_only")["added"] == 30
    assert 0 < mc.reference("partial_growth")["added"] < 30
    assert (mc.reference("nothing")["n"], mc.reference("nothing")["relocated"], mc.reference("nothing")["added"]) == (600, 0, 0)
    assert np.array_equal(mc.reference("nothing")["parents"], np.arange(600))


def test_cases_are_what_the_gpu_tests_assume():
    dom = mc.reference("dominated")
    heavy = int(np.argmax(mc.case("dominated")[0]["op"]))
    assert dom["copies"][heavy] >= 8 and dom["copies"][heavy] + 1 < mcmc_ref.MAX_N
    for name in ("one_alive", "one_alive_opaque"):
        r = mc.reference(name)
        assert int((r["copies"] > 0).sum()) == 1 and r["copies"].max() + 1 > mcmc_ref.MAX_N
    assert mc.reference("one_alive")["rel"]["o_new"][0] == np.float32(mc.MIN_OPACITY)
    assert mc.reference("one_alive_opaque")["rel"]["o_new"][0] == np.float32(1.0 - mcmc_ref.FLT_EPSILON)
    for name in mc.NAMES:
        sc, _ = mc.case(name)
        r = mc.reference(name)
        # quaternions that need their normalisation, scales that differ by axis
        assert np.median(np.abs(np.linalg.norm(sc["quats"], axis=1) - 1.0)) > 0.1 and np.median(sc["scales"].max(axis=1) / sc["scales"].min(axis=1)) > 1.2
        if r["rel"] is not None and name != "one_alive_opaque":
            assert sc["op"][r["rel"]["sources"]].max() <= np.float32(0.99)
    big = mc.reference("big")
    assert len(big["source"]) > 5000 and len(np.unique(big["source"] // 256)) > 250


def test_float32_error_tables_are_current():
    """mcmc_cases.F32_ERR and NOISE_F32_ERR (the GPU bounds are four times them) are what mcmc_ref computes today, every figure within 5 %."""
    now = {name: mc.float32_errors(name) for name in mc.NAMES}
    assert set(mc.F32_ERR) == {k for k, v in now.items() if v is not None}
    for name, row in mc.F32_ERR.items():
        for k, v in row.items():
            assert abs(v - now[name][k]) <= 0.05 * now[name][k], (name, k, v, now[name][k])
    assert set(mc.NOISE_F32_ERR) == set(mc.NOISE_NAMES)
    for name, v in mc.NOISE_F32_ERR.items():
        e = mc.noise_float32_error(name)
        assert e > 0 and abs(v - e) <= 0.05 * e, (name, v, e)


def test_noise_restatement():
    """Opaque Gaussians stay where they are; the key is (seed, step, index): the same key the same normals, another step others; the
    normals are standard."""
    sc = mc.ref_scene(mc.noise_scene("n600_sh3"))
    m = np.asarray(sc["means"], np.float64)
    a = mcmc_ref.noise(sc, **mc.NOISE)
    a32 = mcmc_ref.noise(sc, dtype=np.float32, **mc.NOISE)
    opaque = sc["opacities"] >= 0.5
    assert 100 < opaque.sum() < 500 and a32.dtype == np.float32
    assert np.array_equal(a32[opaque], sc["means"][opaque]) and np.abs(a[opaque] - m[opaque]).max() < 1e-12
    moved = np.abs(a - m).max(axis=1)
    assert (moved[~opaque] > 1e-4).sum() > 100 and moved.max() < 1.0
    assert np.array_equal(a, mcmc_ref.noise(sc, **mc.NOISE)) and not np.array_equal(a, mcmc_ref.noise(sc, **dict(mc.NOISE, step=4)))
    x = mcmc_ref.noise_normals(5, 3, np.arange(8192))
    assert abs(x.mean()) < 0.03 and abs(x.var() - 1.0) < 0.05
    y = mcmc_ref.noise_normals(5, 3, np.arange(8192) + 1)
    assert np.array_equal(x[1:], y[:-1])   # the index is the key, not the position


# ---- the schedule on a recording stand-in --------------------------------------------------------------------------------------------
class Recorder:
    """The methods fit_scene uses, on no scene at all: frames are constants, gradients zeros, a refine or densify call adds ``grow``
    Gaussians; every call is recorded."""

    def __init__(self, n, grow=0):
        self.n, self.grow, self.calls = n, grow, []

    def read_scene(self):
        return dict(means=torch.zeros(self.n, 3, dtype=torch.float64))

    def render(self, V, K, W, H, background=(0.0, 0.0, 0.0), **kw):
        self.calls.append(("render",))
        return dict(rgb=torch.full((H, W, 3), 0.25, dtype=torch.float64), alpha=torch.zeros(H, W, 1, dtype=torch.float64), depth=torch.zeros(H, W, 1, dtype=torch.float64))

    def render_backward(self, V, K, W, H, g_rgb=None, g_alpha=None, g_depth=None, *, out=None, want=None, **kw):
        self.calls.append(("render_backward",))
        res = dict(out or {})
        shapes = dict(means=(self.n, 3), opacities=(self.n,), colors=(self.n, 1, 3), quats=(self.n, 4), scales=(self.n, 3))
        for k in want:
            if res.get(k) is None:
                res[k] = torch.zeros(shapes[k], dtype=torch.float64)
        return res

    def adam_step(self, grads, lrs, step, **kw):
        self.calls.append(("adam_step", step, {k: (tuple(v.shape), float(v.reshape(-1)[0]), float(v.min()), float(v.max())) for k, v in grads.items()}, dict(lrs), kw))

    def mcmc_refine(self, **cfg):
        self.calls.append(("mcmc_refine", cfg))
        self.n += self.grow
        return dict(n=self.n, relocated=2, added=self.grow)

    def mcmc_noise(self, scale, step, seed=0):
        self.calls.append(("mcmc_noise", scale, step, seed))

    def new_density_stats(self):
        return dict(grad_sum=torch.zeros(self.n), count=torch.zeros(self.n, dtype=torch.int32), max_radius=torch.zeros(self.n))

    def density_accumulate(self, W, H, stats, d_means2d=None):
        self.calls.append(("density_accumulate",))

    def densify(self, stats, **cfg):
        self.calls.append(("densify", cfg))
        self.n += self.grow
        return dict(n=self.n)

    def reset_opacity(self, max_opacity=0.01):
        self.calls.append(("reset_opacity", max_opacity))


WHAT = ("means", "opacities", "scales", "colors")


def _run(densify, grow=0, iters=12, what=WHAT, **kw):
    rng = np.random.default_rng(1)
    V, K = rng.normal(size=(3, 4, 4)).astype(np.float32), rng.normal(size=(3, 3, 3)).astype(np.float32)
    R = Recorder(10, grow)
    res = fit.fit_scene(None, V, K, 4, 2, np.zeros((3, 2, 4, 3), np.float32), iters, what=what, views_per_step=2, renderer=R, densify=densify,
                        extent=2.5, **kw)
    return R, res


def test_fit_scene_schedule_on_a_recording_stand_in():
    cfg = fit.McmcConfig(cap_max=99, start=3, stop=11, every=2, min_opacity=0.01, grow_factor=1.5, noise_lr=100.0, opacity_reg=0.02, scale_reg=0.03, seed=3)
    assert [t for t in range(1, 13) if cfg.refine_at(t)] == [4, 6, 8, 10]   # start < t < stop: gsplat's rule
    assert not fit.McmcConfig(cap_max=1).refine_at(500) and fit.McmcConfig(cap_max=1).refine_at(600) and not fit.McmcConfig(cap_max=1).refine_at(25000)
    R, res = _run(cfg, grow=7)
    names = [c[0] for c in R.calls]
    assert "density_accumulate" not in names and "densify" not in names and "reset_opacity" not in names   # no statistics are kept
    step_at = lambda k: [c for c in R.calls[:k] if c[0] == "adam_step"][-1][1]
    ref = [k for k, c in enumerate(R.calls) if c[0] == "mcmc_refine"]
    assert [step_at(k) for k in ref] == [4, 6, 8, 10] and all(names[k - 1] == "adam_step" and names[k + 1] == "mcmc_noise" for k in ref)
    assert [R.calls[k][1] for k in ref] == [dict(min_opacity=0.01, cap_max=99, grow_factor=1.5, seed=3 + t) for t in (4, 6, 8, 10)]
    # noise after every step, behind the step (and the refine): noise_lr times the means' decayed rate
    noise = [c for c in R.calls if c[0] == "mcmc_noise"]
    assert [c[2] for c in noise] == list(range(1, 13)) and all(c[3] == 3 for c in noise)
    for c in noise:
        want = 100.0 * fit.step_rates(fit.DEFAULT_LRS, WHAT, 2.5, c[2], 12)["means"]
        assert c[1] == pytest.approx(want, rel=1e-12) and want > 0
    assert noise[0][1] > 50 * noise[-1][1]   # (the rate decays to a hundredth)
    assert [names[k + 1] for k, c in enumerate(R.calls) if c[0] == "adam_step" and k + 1 not in ref] == ["mcmc_noise"] * 8
    # the regularisers: constants at the CURRENT N (the recorder's own gradients are zeros), only on opacities and scales
    steps = {c[1]: c for c in R.calls if c[0] == "adam_step"}
    n_at = [10] * 4 + [17] * 2 + [24] * 2 + [31] * 2 + [38] * 2
    for t in range(1, 13):
        g = steps[t][2]
        n = n_at[t - 1]
        assert g["opacities"][0] == (n,) and g["scales"][0] == (n, 3)
        assert g["opacities"][2] == g["opacities"][3] == pytest.approx(0.02 / n, rel=1e-12)
        assert g["scales"][2] == g["scales"][3] == pytest.approx(0.03 / (3 * n), rel=1e-12)
        assert g["means"][2] == g["means"][3] == 0.0 and g["colors"][2] == g["colors"][3] == 0.0
        assert steps[t][3] == fit.step_rates(fit.DEFAULT_LRS, WHAT, 2.5, t, 12)
    assert res.n_history == [10] * 3 + [17] * 2 + [24] * 2 + [31] * 2 + [38] * 3 and res.steps == 12
    assert res.refines == [(4, 17, 2, 7), (6, 24, 2, 7), (8, 31, 2, 7), (10, 38, 2, 7)]   # (step, N, relocated, added) of every refine
    # noise_lr = 0 and no regularisers: the refine alone
    R0, _ = _run(fit.McmcConfig(cap_max=99, start=3, stop=11, every=2, noise_lr=0.0, opacity_reg=0.0, scale_reg=0.0), what=("colors", "opacities"))
    assert "mcmc_noise" not in [c[0] for c in R0.calls] and sum(c[0] == "mcmc_refine" for c in R0.calls) == 4
    assert all(c[2]["opacities"][2:] == (0.0, 0.0) for c in R0.calls if c[0] == "adam_step")


def test_without_mcmc_the_loop_is_the_one_it_was():
    plain, res0 = _run(None)
    assert [c[0] for c in plain.calls] == ["render", "render_backward", "render", "render_backward", "adam_step"] * 12 and res0.n_history == [] and res0.refines == []
    assert all(c[2]["opacities"][2:] == (0.0, 0.0) and c[2]["scales"][2:] == (0.0, 0.0) for c in plain.calls if c[0] == "adam_step")
    dens, res1 = _run(fit.DensifyConfig(start=4, stop=11, every=2, reset_every=5, max_gaussians=99, seed=3), grow=7)
    per_step = ["render", "render_backward", "density_accumulate", "render", "render_backward", "density_accumulate", "adam_step"]
    want = []
    for t in range(1, 13):
        want += per_step + (["densify"] if t in (4, 6, 8, 10) else []) + (["reset_opacity"] if t in (5, 10) else [])
    assert [c[0] for c in dens.calls] == want and res1.n_history == [10] * 3 + [17] * 2 + [24] * 2 + [31] * 2 + [38] * 3 and res1.refines == []
    assert all(c[2]["opacities"][2:] == (0.0, 0.0) for c in dens.calls if c[0] == "adam_step")
    sent = [c[1] for c in dens.calls if c[0] == "densify"]
    assert [s["seed"] for s in sent] == [7, 9, 11, 13] and all(s["max_gaussians"] == 99 and s["scene_extent"] == 2.5 for s in sent)


def test_validation_in_python():
    for bad in (dict(cap_max=0), dict(every=0), dict(start=-1), dict(min_opacity=1.0), dict(min_opacity=float("nan")), dict(grow_factor=0.9),
                dict(grow_factor=float("inf")), dict(noise_lr=-1.0), dict(opacity_reg=float("nan")), dict(scale_reg=-0.1)):
        with pytest.raises(ValueError, match="McmcConfig"):
            _run(fit.McmcConfig(**dict(dict(cap_max=50), **bad)))
    with pytest.raises(ValueError, match="noise_lr"):
        _run(fit.McmcConfig(cap_max=50), what=("colors", "opacities"))

    # a stand-in renderer without the two methods is told so before anything runs
    bare = type("Bare", (), {k: getattr(Recorder, k) for k in ("read_scene", "render", "render_backward", "adam_step")})()
    bare.n, bare.calls = 10, []
    with pytest.raises(ValueError, match="mcmc_refine"):
        fit.fit_scene(None, np.zeros((1, 4, 4), np.float32), np.zeros((1, 3, 3), np.float32), 4, 2, np.zeros((1, 2, 4, 3), np.float32), 2, what=WHAT,
                      renderer=bare, densify=fit.McmcConfig(cap_max=50), extent=1.0)
    assert bare.calls == []
    # Rasterizer.mcmc_refine refuses unknown settings before it touches the library
    with pytest.raises(ValueError, match="unknown settings"):
        Rasterizer.mcmc_refine.__wrapped__(type("R", (), dict(_MCMC_CONFIG=Rasterizer._MCMC_CONFIG))(), cap=5)
