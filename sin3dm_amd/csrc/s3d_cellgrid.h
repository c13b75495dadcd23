// s3d_cellgrid.h — the uniform cell grid that s3d_meshsdf.hip bins triangles into and that s3d_ray.hip walks:
// one definition of the grid and of the cell of a coordinate, so that the binning and the walk cannot disagree about a border.
#pragma once
#include "s3d_common.h"

namespace s3d {

struct CellGrid { float ox, oy, oz, cell; int nx, ny, nz; };

// the cell of a coordinate along one axis, clamped to the grid: monotone in x, so a range of coordinates maps to a range of cells
__device__ __forceinline__ int cell_of(float x, float o, float cell, int n) {
    return min(n - 1, max(0, int(floorf(__fdiv_rn(x - o, cell)))));
}

}  // namespace s3d
