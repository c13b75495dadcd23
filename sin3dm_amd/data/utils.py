"""Host half of the preprocessing: the reference's data/utils.py in float64, arithmetic and quirks kept (the aabb that
normalize_aabb first computes from the vertices is discarded: the one it returns is +-fm_size / fm_size.max())."""
import numpy as np


def sample_grid_points_aabb(aabb, resolution):
    """Cell centres of the grid with `resolution` cells along the longest aabb axis: (Nx, Ny, Nz, 3) float64."""
    aabb = np.asarray(aabb, dtype=np.float64)
    aabb_min, aabb_max = aabb[:3], aabb[3:]
    aabb_size = aabb_max - aabb_min
    resolutions = (resolution * aabb_size / aabb_size.max()).astype(np.int32)
    axes = [np.linspace(0.5, resolutions[k] - 0.5, resolutions[k]) / resolutions[k] * aabb_size[k] + aabb_min[k] for k in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)


def normalize_aabb(v, reso, enlarge_scale=1.03, mult=8):
    """(aabb, translation, scale): v -> (v + translation) * scale puts the longest bounding-box axis into [-1, 1] / enlarge_scale;
    aabb = [-m, m] with m = fm_size / fm_size.max(), fm_size the per-axis grid size at `reso` rounded up to a multiple of `mult`."""
    v = np.asarray(v, dtype=np.float64)
    aabb_min = np.min(v, axis=0)
    aabb_max = np.max(v, axis=0)
    center = (aabb_max + aabb_min) / 2
    bbox_size = (aabb_max - aabb_min).max() * enlarge_scale
    translation = -center
    scale = 1.0 / bbox_size * 2
    aabb_min = (aabb_min * enlarge_scale - center) / bbox_size * 2
    aabb_max = (aabb_max * enlarge_scale - center) / bbox_size * 2
    aabb_size = aabb_max - aabb_min
    fm_size = (reso * aabb_size / aabb_size.max()).astype(np.int32)
    fm_size = (fm_size + mult - 1) // mult * mult
    aabb_max = fm_size / fm_size.max()
    return np.concatenate([-aabb_max, aabb_max], axis=0), translation, scale
