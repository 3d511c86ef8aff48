"""Child process of tests/test_gpu_zf_skin_rest.py: ``deform_backward_rest`` of its cases under the SAS_SKIN_LDS of its environment (the
knob is read when the library's context is made), saved for the parent to compare bit for bit.

    python tests/tools/skin_rest_child.py OUT.npz

Saves ``<case>_<form>_<array>`` = the rest gradients, per case of CASES."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import skin_rest_ref as rr  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402

CASES = [(name, form) for name in rr.CASES for form in rr.FORMS]


def rest_grad(r, c, means=True, orient=True, bound_only=False, out=None):
    """``deform_backward_rest`` of case ``c`` on rasterizer ``r``, the binding set as the kit holds it (the parent runs the same function
    under the default budget); returns the result's device tensors."""
    r.upload(**c["scene"])
    r.set_skin(c["indices"], c["weights"])
    r.deform(c["transforms"])
    grads = {}
    if means:
        grads["means"] = torch.from_numpy(c["d_means"]).to(r.device)
    if orient:
        grads[c["form"]] = torch.from_numpy(c["d_orient"]).to(r.device)
    return r.deform_backward_rest(grads, out=out, bound_only=bound_only)


def main(out):
    r = Rasterizer(0)
    res = {}
    for name, form in CASES:
        for a, v in rest_grad(r, rr.case(name, form)).items():
            res[f"{name}_{form}_{a}"] = v.cpu().numpy()
    r.close()
    np.savez(out, **res)
    print("skin rest child ok")


if __name__ == "__main__":
    main(sys.argv[1])
