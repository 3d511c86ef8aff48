"""GPU: a slice of the observation fuzzer (tests/tools/obs_fuzz.py) in the suite -- per arm the committed seeds of OBS_SEEDS, drawn
scenes and cameras (odd cameras, strips, poisoned Gaussians, depth planes, 1-40 posed groups) through render_rgbd,
render_cameras_host, render_batch_labels, lift_labels and render_batch_labels + sample_point_cloud; every output equal to an
expectation formed from the C oracle, cloud_ref, lift_ref and NumPy alone (floats bit for bit).  That the seeds reach the edges they
are there for is settled on the CPU (tests/test_obs_fuzz_cpu.py).  The file runs unchanged under the bounds-checked build.
Long runs: `python tests/tools/obs_fuzz.py 1500`, `python tests/tools/obs_fuzz.py 300 5000 poison-all` (profiles/obs_fuzz.txt)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import obs_fuzz as of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arm", of.ARMS)
def test_drawn_cases_equal_their_references(rasterizer, arm):
    assert 10 <= len(of.OBS_SEEDS[arm]) <= 12
    for seed in of.OBS_SEEDS[arm]:
        c = of.draw_case(seed)
        assert c["arm"] == arm, of.describe(c)
        diffs = of.run_case(rasterizer, c)
        assert not diffs, (of.describe(c), diffs)


@pytest.mark.parametrize("seed, poison_all", of.LIFT_SEEDS_OPACITY_NOT_FINITE)
def test_lift_case_with_an_opacity_that_is_not_finite(rasterizer, seed, poison_all):
    """A Gaussian with opacity NaN or +Inf is composited with alpha 0.999 wherever it is listed: the lanes of a ragged tile that lie
    beyond the image must still give it nothing."""
    c = of.draw_case(seed, poison_all)
    assert c["arm"] == "lift" and not np.isfinite(c["scene"].opacities).all() and (c["W"] % 16 or c["H"] % 16)
    diffs = of.run_case(rasterizer, c)
    assert not diffs, (of.describe(c), diffs)


@pytest.mark.parametrize("opacity", [np.inf, np.nan])
def test_reduced_lift_case(rasterizer, opacity):
    sc, cam, labels, n_labels = of.reduced_lift_case(opacity)
    V, K, W, H = cam
    want = of.lift_ref.reference(sc, cam, labels[0], n_labels)
    of.lift_ref.sc_kit.upload(rasterizer, sc)
    o = rasterizer.lift_labels(V[None], K[None], W, H, labels, n_labels)
    diffs = of.compare({k: v.cpu().numpy() for k, v in o.items()}, dict(votes=want[0], seen=want[1]))
    assert not diffs, diffs
