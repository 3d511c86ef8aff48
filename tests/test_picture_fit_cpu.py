"""CPU: what the picture-fitting loops share (sim_a_splat_amd/_picture_fit.py; DESIGN.md 3, "Backward pass" and "Deformation") against the
formulas written out here, bit for bit: the Adam rule on twists and its three scalars, one level of the image pyramid, and the host stepper
of the node fits against rigidity + _twist_step called by hand."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import skin_ref as sr  # noqa: E402

from sim_a_splat_amd import _picture_fit as pf  # noqa: E402
from sim_a_splat_amd import deform  # noqa: E402

STEP = (0.01, 0.02)


@pytest.mark.parametrize("n", [1, 3, 9])
@pytest.mark.parametrize("per", [1, 5])
def test_twist_adam_is_the_rule_written_out_per_row(n, per):
    """A chain of 5 steps from zero moments (``it = 0`` first; with ``per = 1`` the decay's denominator is clamped), one gradient row zero
    throughout: every row of every step is the scalar-loop form of the rule, bit for bit."""
    rng = np.random.default_rng(100 + n)
    m1, m2 = np.zeros((n, 6)), np.zeros((n, 6))
    r1, r2 = np.zeros((n, 6)), np.zeros((n, 6))
    for it in range(5):
        tw = rng.normal(0.0, 10.0 ** rng.uniform(-6, 0), (n, 6))
        tw[n // 2] = 0.0
        xi, m1, m2 = pf.twist_adam(tw, m1, m2, it, per, STEP)
        assert xi.shape == m1.shape == m2.shape == (n, 6) and xi.dtype == np.float64
        for q in range(n):
            g = tw[q]
            r1[q] = 0.9 * r1[q] + 0.1 * g
            r2[q] = 0.999 * r2[q] + 0.001 * g * g
            hat = (r1[q] / (1 - 0.9 ** (it + 1))) / (np.sqrt(r2[q] / (1 - 0.999 ** (it + 1))) + 1e-12)
            decay = 0.05 ** (it / max(1, per - 1))
            want = -np.concatenate([STEP[0] * decay * hat[:3], STEP[1] * decay * hat[3:]])
            assert np.array_equal(xi[q], want), (it, q)
        assert np.array_equal(m1, r1) and np.array_equal(m2, r2)
        assert not xi[n // 2].any() and (n == 1 or xi.any())   # a zero gradient moves nothing


def test_adam_scalars_are_the_three_expressions():
    for it, per in [(0, 1), (0, 2), (1, 2), (4, 5), (7, 100), (99, 100), (299, 100)]:
        assert pf.adam_scalars(it, per) == (0.05 ** (it / max(1, per - 1)), 1 - 0.9 ** (it + 1), 1 - 0.999 ** (it + 1))
    assert pf.adam_scalars(0, 1)[0] == 1.0 and pf.adam_scalars(4, 5)[0] == 0.05


def _drawn_views(c, h, w, seed):
    rng = np.random.default_rng(seed)
    imgs = torch.from_numpy(rng.uniform(0, 1, (c, h, w, 3)).astype(np.float32))
    ms = torch.from_numpy((rng.uniform(0, 1, (c, h, w)) > 0.4).astype(np.float32))
    ms[0, :4, :6] = 0.0   # a block without coverage: the renormalisation's clamp
    K = np.stack([np.array([[20.0 + v, 0.3, 8.0 + v], [0.0, 21.0, 6.0 - v], [0.0, 0.0, 1.0]]) for v in range(c)])
    return imgs, ms, K


def test_pyramid_at_factor_one_returns_its_inputs():
    imgs, ms, K = _drawn_views(3, 12, 16, 7)
    w, h, targets, tms, Kcs = pf.pyramid_level(imgs, ms, K, 16, 12, 1)
    assert (w, h) == (16, 12) and targets is imgs and tms is ms
    assert np.array_equal(Kcs, K) and Kcs is not K


def test_pyramid_at_factor_two_is_the_per_image_computation():
    W, H = 16, 12
    imgs, ms, K = _drawn_views(3, H, W, 8)
    w, h, targets, tms, Kcs = pf.pyramid_level(imgs, ms, K, W, H, 2)
    assert (w, h) == (8, 6) and tuple(targets.shape) == (3, 6, 8, 3) and tuple(tms.shape) == (3, 6, 8) and tms.dtype == torch.float32
    for v in range(3):
        img, m = imgs[v], ms[v]
        cover = Fn.interpolate(m[None, None], size=(h, w), mode="area")[0, 0]
        target = Fn.interpolate((img * m[..., None]).permute(2, 0, 1)[None], size=(h, w), mode="area")[0].permute(1, 2, 0) / torch.clamp(cover, min=1e-6)[..., None]
        assert torch.equal(targets[v], target) and torch.equal(tms[v], (cover > 0.5).to(torch.float32))
        Kc = K[v].copy()
        Kc[0] *= w / W
        Kc[1] *= h / H
        assert np.array_equal(Kcs[v], Kc) and np.array_equal(Kcs[v, 2], K[v, 2])
    assert not tms[0, :2, :3].any() and not targets[0, :2, :3].any() and 0 < float(tms.sum()) < tms.numel()
    one = pf.pyramid_level(imgs[:1], ms[:1], K[:1], W, H, 2)   # one image alone: the batch's first
    assert torch.equal(one[2][0], targets[0]) and torch.equal(one[3][0], tms[0]) and np.array_equal(one[4][0], Kcs[0])


@pytest.mark.parametrize("weight", [0.01, 0.0])
def test_host_stepper_is_rigidity_and_twist_step_by_hand(weight):
    """Three steps on a 3x3 grid from a bent start: the stepper's transforms, moments and returned rigidity value against ``rigidity`` (its
    own neighbour search) and ``_twist_step`` called by hand; with a weight of 0 the value is an exact 0.0 and no rigidity gradient is added."""
    nodes = deform.grid_nodes(((-0.5, -0.5, 0.0), (0.5, 0.5, 0.0)), 0.5).astype(np.float64)
    assert nodes.shape == (9, 3)
    T = sr.transforms(nodes, angle=0.3).astype(np.float64)
    rng = np.random.default_rng(11)
    opt = deform._HostNodes(nodes, T.copy())
    assert opt.transforms.dtype == np.float32 and opt.transforms.flags["C_CONTIGUOUS"] and np.array_equal(opt.transforms, T.astype(np.float32))
    assert opt.transforms64.dtype == np.float64 and np.array_equal(opt.read(), T)
    m1, m2 = np.zeros((9, 6)), np.zeros((9, 6))
    for it in range(3):
        d = rng.normal(0.0, 1e-3, (9, 3, 4))
        got = opt.step(torch.from_numpy(d.astype(np.float32)) if it == 1 else d, it, 3, STEP, weight)
        if it == 1:
            d = d.astype(np.float32).astype(np.float64)
        value, d_reg = deform.rigidity(nodes, T)
        T, m1, m2 = deform._twist_step(T, d + weight * d_reg if weight > 0.0 else d, nodes, m1, m2, it, 3, STEP)
        assert (got == value and value > 0.0) if weight > 0.0 else (type(got) is float and got == 0.0)
        assert np.array_equal(opt.read(), T) and np.array_equal(opt.m1, m1) and np.array_equal(opt.m2, m2)
        assert np.array_equal(opt.transforms, np.ascontiguousarray(T.astype(np.float32)))
        now, ref = opt.rigidity(), deform.rigidity(nodes, T)   # the table made once against the search of every call
        assert now[0] == ref[0] and np.array_equal(now[1], ref[1])
    opt.reset_moments()
    assert not opt.m1.any() and not opt.m2.any() and np.array_equal(opt.read(), T)
