"""Child process of tests/test_gpu_zd_skin.py: the deformed scenes of its cases under the SAS_SKIN_LDS of its environment (the knob is read
when the library's context is made), saved for the parent to compare bit for bit.

    python tests/tools/skin_child.py OUT.npz

Saves ``<form>_<nodes>_k<k>_<array>`` = read_scene()'s arrays after bind_skin + deform, per case of CASES."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import skin_ref as sr  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402

CASES = [(form, name, k) for form in ("quats", "covariances") for name, k in (("m3", 1), ("m70", 4), ("m70", 8), ("m256", 4), ("m300", 8))]


def deformed(r, form, name, k):
    """read_scene() as numpy after the case's bind and deformation (the parent runs the same function under the default budget)."""
    q = sr.nodes(name)
    r.upload(**sr.scene(form))
    r.bind_skin(q, k=k)
    r.deform(sr.transforms(q))
    return {a: t.cpu().numpy() for a, t in r.read_scene().items()}


def main(out):
    r = Rasterizer(0)
    res = {}
    for form, name, k in CASES:
        for a, v in deformed(r, form, name, k).items():
            res[f"{form}_{name}_k{k}_{a}"] = v
    r.close()
    np.savez(out, **res)
    print("skin child ok")


if __name__ == "__main__":
    main(sys.argv[1])
