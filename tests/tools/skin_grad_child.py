"""Child process of tests/test_gpu_ze_skin_grad.py: ``deform_backward`` of its cases under other settings of SAS_SKIN_GRAD_LDS and
SAS_SKIN_GRAD_STAGED than the defaults (the knobs are read when the library's context is made: one context per setting), saved for the
parent to compare.

    python tests/tools/skin_grad_child.py OUT.npz

Saves ``<setting>_<case>_<form>`` = the gradient [m,3,4], per setting of SETTINGS and case of CASES."""
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import skin_grad_ref as sg  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402

# name -> environment: every sum in global memory (rows staged); the rows staged on both paths; every lane adding its own row on both paths
SETTINGS = {"global": {"SAS_SKIN_GRAD_LDS": "0"}, "staged": {"SAS_SKIN_GRAD_STAGED": "1"}, "direct": {"SAS_SKIN_GRAD_STAGED": "0"}}
CASES = [(name, form) for name in ("m1", "m5_k3", "m70_k4", "m257_k8", "m2048_k4", "m2049_k4") for form in sg.FORMS]


def node_grad(r, c, means=True, orient=True):
    """``deform_backward`` of case ``c`` on rasterizer ``r`` as numpy (the parent runs the same function under the defaults)."""
    r.upload(**c["scene"])
    r.set_skin(c["indices"], c["weights"])
    r.deform(c["transforms"])
    grads = {}
    if means:
        grads["means"] = torch.from_numpy(c["d_means"]).to(r.device)
    if orient:
        grads[c["form"]] = torch.from_numpy(c["d_orient"]).to(r.device)
    return r.deform_backward(grads).cpu().numpy()


def main(out):
    res = {}
    for setting, env in SETTINGS.items():
        for k in ("SAS_SKIN_GRAD_LDS", "SAS_SKIN_GRAD_STAGED"):
            os.environ.pop(k, None)
        os.environ.update(env)
        r = Rasterizer(0)
        for name, form in CASES:
            res[f"{setting}_{name}_{form}"] = node_grad(r, sg.case(name, form))
        r.close()
    np.savez(out, **res)
    print("skin grad child ok")


if __name__ == "__main__":
    main(sys.argv[1])
