"""GPU: a slice of the differential fuzzer (tests/tools/oracle_fuzz.py) in the suite -- the first drawn scenes / cameras / entry points,
at least 40 and until every entry point, every SH degree and a poisoned scene have come up; every output bit-equal to the C oracle.
Long runs: `python tests/tools/oracle_fuzz.py 4000` (profiles/r05_oracle_fuzz.txt).

The second test draws meshes into the cases (draw_mesh_case): 40 fixed seeds, each bit-equal to oracle.mesh_ref + the depth-limited
oracle on its stable pixels; which seeds, and that their excluded share stays within 10 %, is settled on the CPU
(tests/test_mesh_ref_cpu.py).  Long runs: `python tests/tools/oracle_fuzz.py --meshes 400` (profiles/mesh_oracle_gpu_suite.txt)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import oracle_fuzz as fz  # noqa: E402

pytestmark = pytest.mark.gpu
ARMS = {"single", "batch", "posed", "host", "pipelined"}


def test_drawn_cases_are_bit_equal_to_the_oracle(rasterizer):
    entries, degrees, poisoned, seed = set(), set(), 0, 0
    while seed < 40 or not (entries == ARMS and degrees == {-1, 0, 1, 2, 3} and poisoned):
        assert seed < 150, (entries, degrees, poisoned)       # the draw reaches every arm long before
        c = fz.draw_case(seed)
        diffs = fz.run_case(rasterizer, c)
        assert not diffs, (fz.describe(c), diffs)
        entries.add(c["entry"]); degrees.add(c["deg"]); poisoned += c["poisoned"]
        seed += 1


def test_drawn_mesh_cases_are_bit_equal_on_stable_pixels(rasterizer):
    assert len(fz.MESH_FUZZ_SEEDS) == 40
    entries, poisoned_vertices = set(), 0
    try:
        for seed in fz.MESH_FUZZ_SEEDS:
            c = fz.draw_mesh_case(seed)
            diffs, excluded = fz.run_mesh_case(rasterizer, c)
            print(fz.describe_mesh(c), f"excluded={100 * excluded:.2f} %")
            assert excluded <= fz.MESH_MAX_EXCLUDED, (fz.describe_mesh(c), excluded)
            assert not diffs, (fz.describe_mesh(c), diffs)
            entries.add(c["entry"]); poisoned_vertices += c["mesh"]["poisoned_vertices"]
        assert {"single", "batch", "host"} <= entries and poisoned_vertices
    finally:
        rasterizer.clear_meshes()


@pytest.mark.parametrize("seed", fz.MESH_SEEDS_VERTEX_AT_1E30)
def test_mesh_case_with_a_vertex_at_1e30(rasterizer, seed):
    """The far end of an edge projects 1e30 px away: the edge must still pass the frame where the reference puts it."""
    c = fz.draw_mesh_case(seed)
    v = c["mesh"]["verts"]
    assert (np.isfinite(v) & (np.abs(v) > 1e20)).any()
    try:
        diffs, excluded = fz.run_mesh_case(rasterizer, c)
        assert excluded <= fz.MESH_MAX_EXCLUDED and not diffs, (fz.describe_mesh(c), excluded, diffs)
    finally:
        rasterizer.clear_meshes()
