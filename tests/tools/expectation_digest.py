"""One line per case and view of the mesh test kit: the counts of mesh_cases.report and a sha256 (first 16 hex digits) of every array
of the expectation.  CPU only.  Run it before and after a change to oracle/mesh_ref.py or tests/tools/*_cases.py: equal output means
the GPU tests are held to the same bits.

    python tests/tools/expectation_digest.py > listing.txt
"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_cases as mc  # noqa: E402
import mesh_feature_cases as mf  # noqa: E402
import mesh_smooth_cases as ms  # noqa: E402
import oracle_fuzz as fz  # noqa: E402

MAPS = ("stable", "cut", "length", "zlim")
REF = ("winner", "z", "delta", "color", "tri_color")
SMOOTH = ("smooth_pixel", "beta", "color64")
smooth_expected = getattr(ms, "expected", mc.expected)          # (before the kits were merged the smooth cases had an `expected` of their own ...
fuzz_expected = (lambda c, i: mc.expected(fz.as_case(c), i)) if hasattr(fz, "as_case") else fz.mesh_reference      # ... and so had the fuzzer)


def digest(e, maps=MAPS, ref=()):
    arrays = [(f"frame.{k}", e["frame"][k]) for k in mc.OUTS] + [(k, e[k]) for k in maps] + [(f"ref.{k}", e["ref"][k]) for k in ref]
    return " ".join(f"{k}={hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]}" for k, a in arrays)


def main():
    fixed = [(n, b, mc.expected, REF, None) for n, b in mc.FIXED_CASES.items()]
    fixed += [(f"smooth_{n}", b, smooth_expected, REF + SMOOTH, None) for n, b in ms.FIXED_CASES.items()] + [("labels", mf.case_labels, mc.expected, REF, None)]
    fixed += [(f"drawn_{s}", lambda s=s: mf.drawn_case(s), mc.expected, REF, 1) for s in mf.DRAWN_SEEDS]      # (the feature tests take the first view)
    for name, build, expected, ref, views in fixed:
        case = build()
        for view in range(views or len(case["cams"])):
            e = expected(case, view)
            print(mc.report(f"{name}[{view}]", case, e), digest(e, ref=ref), flush=True)
    for seed in fz.MESH_FUZZ_SEEDS + fz.MESH_SEEDS_VERTEX_AT_1E30:
        c = fz.draw_mesh_case(seed)
        for view in range(len(c["cams"])):
            e = fuzz_expected(c, view)
            print(f"fuzz_{seed}[{view}]: excluded={e['excluded']!r} covered={e['covered']!r}", digest(e, maps=("stable",)), flush=True)


if __name__ == "__main__":
    main()
