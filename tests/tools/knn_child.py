"""Child process of tests/test_gpu_zc_knn.py: the library's kNN of every test cloud under the SAS_KNN_GRID of its environment (the knob
is read when the library's context is made), saved for the parent to compare bit for bit.

    python tests/tools/knn_child.py OUT.npz

Saves ``<cloud>_dist2``, ``<cloud>_index`` (k = 3) and ``<cloud>_stats`` = (leftover, nx, ny, nz, brute) per cloud."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import knn_ref as kr  # noqa: E402
from sim_a_splat_amd.rasterizer import Rasterizer  # noqa: E402


def main(out):
    r = Rasterizer(0)
    res = {}
    for name in kr.ALL_CLOUDS:
        got = r.knn_points(torch.from_numpy(kr.cloud(name)).to(r.device), 3)
        st = r.knn_stats()   # (blocking: the call is complete)
        res[f"{name}_dist2"] = got["dist2"].cpu().numpy()
        res[f"{name}_index"] = got["index"].cpu().numpy()
        res[f"{name}_stats"] = np.array([st["leftover"], *st["grid"], int(st["brute"])], np.int64)
    r.close()
    np.savez(out, **res)
    print("knn child ok")


if __name__ == "__main__":
    main(sys.argv[1])
