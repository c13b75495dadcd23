"""The procedural volumes and cases of the geometry-evaluation tests, shared by tests/test_eval_gpu.py, tests/test_eval_host.py
and the fixture generator tests/golden/make_golden_eval.py.  tests/golden/eval_geometry.npz stores parameters and results only:
every volume is regenerated from the formulas here."""
import numpy as np

from sin3dm_amd.testing import gyroid_sdf

# name: (shape, freq, phase)
VOLUMES = {
    "ref48": ((48, 40, 36), 2.5, (0.0, 0.0, 0.0)),
    "gen48a": ((48, 40, 36), 2.5, (0.4, 0.1, -0.3)),
    "gen48b": ((48, 40, 36), 2.5, (-0.2, 0.5, 0.25)),
    "ref32": ((32, 26, 20), 1.5, (0.0, 0.0, 0.0)),
    "gen32a": ((32, 26, 20), 1.5, (0.02, -0.01, 0.01)),
    "ref40": ((40, 33, 25), 1.5, (0.0, 0.0, 0.0)),
    "gen40a": ((40, 33, 25), 1.5, (0.3, -0.2, 0.1)),
    "gen40b": ((40, 33, 25), 1.5, (-0.15, 0.35, 0.2)),
    "div0": ((32, 26, 20), 1.5, (0.0, 0.0, 0.0)),
    "div1": ((32, 26, 20), 1.5, (0.3, -0.2, 0.1)),
    "div2": ((32, 26, 20), 1.5, (-0.4, 0.2, 0.6)),
    "div3": ((32, 26, 20), 2.0, (0.1, 0.7, -0.5)),
    "div4": ((32, 26, 20), 1.0, (0.9, 0.0, 0.3)),
}

# name: (reference volume, generated volumes in order, patch_size, stride, patch_num, resolution).  A generated name equal to the
# reference's means the identical occupancy (sdf <= 0); the others are sdf < 0, as the decoders write them.
LP_CASES = {
    "p11_48": ("ref48", ("gen48a", "gen48b"), 11, 5, 300, 48),          # odd patch, ragged last word, shuffle taken, stream carries over
    "p6_48": ("ref48", ("gen48a", "gen48b"), 6, None, 1000, 48),        # even patch, default stride, > 1000 reference patches
    "p11_32": ("ref32", ("gen32a", "ref32"), 11, 5, 1000, 32),          # n_gen < patch_num; an identical shape: everything 1.0
    "p11_pool": ("ref40", ("gen40a", "gen40b"), 11, 5, 1000, 32),       # (40, 33, 25) pooled to (32, 26, 20): non-integer windows
}
POOL_KEYS = {"gen40a": "vox_grid", "gen40b": "voxel"}                   # the two keys load_voxgrid reads
POOL_UP = ("gen32a", 40)                                                # (32, 26, 20) pooled up to (40, 32, 25)
DIV_CASE = ("div0", "div1", "div2", "div3", "div4")
DIV_RESOLUTION = 32


def sdf(name):
    shape, freq, phase = VOLUMES[name]
    return gyroid_sdf(shape, freq, phase)


def reference_occupancy(name):
    """The training shape's rule: occupied where sdf <= 0."""
    return sdf(name) <= 0


def generated_occupancy(name, ref_name=None):
    """The decoders' rule, sdf < 0; the reference's own name gives the reference's occupancy exactly."""
    return reference_occupancy(name) if name == ref_name else sdf(name) < 0


def write_case_files(case, directory):
    """The case as files: (paths of the generated shapes, path of the reference), keys as the project writes them."""
    import os
    ref_name, gens, *_ = LP_CASES[case]
    ref_path = os.path.join(directory, f"{case}_ref.npz")
    np.savez(ref_path, sdf_grid=sdf(ref_name))
    paths = []
    for i, g in enumerate(gens):
        path = os.path.join(directory, f"{case}_gen{i}_voxel.npz")
        np.savez(path, **{POOL_KEYS.get(g, "vox_grid"): generated_occupancy(g, ref_name)})
        paths.append(path)
    return paths, ref_path
