"""Writes tests/golden/prepare_host.npz: what the reference's data/utils.py (NumPy only) returns for a handful of vertex sets and
(reso, mult, enlarge_scale) triples — normalize_aabb's (aabb, translation, scale) and sample_grid_points_aabb's grid axes.

    python tests/golden/make_golden_prepare.py /path/to/reference

One vertex set holds the eight bounding-box corners of the reference's towerruins OBJ (its aabb depends on nothing else)."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TOWERRUINS_BBOX = ((-2.273209, 0.016134, -2.333855), (2.290273, 6.337532, 2.209331))       # min / max of the `v` lines of mesh/model.obj


def vertex_sets():
    rng = np.random.Generator(np.random.PCG64(2024))
    lo, hi = (np.asarray(x) for x in TOWERRUINS_BBOX)
    corners = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])
    return {"towerruins_bbox": corners,
            "cube": rng.uniform(-1, 1, size=(50, 3)),
            "slab": rng.uniform(-1, 1, size=(64, 3)) * np.array([3.0, 0.4, 1.7]) + np.array([10.0, -4.0, 0.25]),
            "needle": rng.normal(size=(40, 3)) * np.array([0.3, 2.0, 0.6]),
            "offset": rng.uniform(0, 1, size=(30, 3)) * np.array([1.0, 0.77, 0.51]) + 100.0}


CONFIGS = ((256, 8, 1.03), (128, 8, 1.03), (24, 4, 1.03), (32, 8, 1.0), (100, 16, 1.2), (64, 1, 1.03))


def main(reference):
    sys.path.insert(0, os.path.join(reference, "data"))
    import utils as ref                                    # the reference's data/utils.py
    out = {"configs": np.asarray(CONFIGS, dtype=np.float64)}
    for name, v in vertex_sets().items():
        out[f"{name}/verts"] = v
        for i, (reso, mult, enlarge) in enumerate(CONFIGS):
            with contextlib.redirect_stdout(io.StringIO()):
                aabb, translation, scale = ref.normalize_aabb(v, reso, enlarge_scale=enlarge, mult=mult)
                grid = ref.sample_grid_points_aabb(aabb, reso)
            out[f"{name}/{i}/aabb"], out[f"{name}/{i}/translation"], out[f"{name}/{i}/scale"] = aabb, translation, np.float64(scale)
            out[f"{name}/{i}/shape"] = np.asarray(grid.shape, dtype=np.int64)
            out[f"{name}/{i}/xs"], out[f"{name}/{i}/ys"], out[f"{name}/{i}/zs"] = grid[:, 0, 0, 0], grid[0, :, 0, 1], grid[0, 0, :, 2]
            out[f"{name}/{i}/corner"] = grid[-1, -1, -1]
    np.savez_compressed(os.path.join(HERE, "prepare_host.npz"), **out)
    print("towerruins_bbox at reso 256, mult 8:", out["towerruins_bbox/0/aabb"], out["towerruins_bbox/0/shape"])


if __name__ == "__main__":
    main(sys.argv[1])
