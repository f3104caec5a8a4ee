// The cell grid shared by the neighbourhood search (spatial.hip) and the cell graph (graph.hip): both read points in cell order and their
// cell_start (hdy_spatial_cells, include/hdyolo_spatial.h), so the grid, a point's cell, a grid row's run of points and the argument checks
// of `pts`, the grid and `cell_start` exist once.  Everything is local to the including file (other files have a Grid of their own).
#pragma once
#include "common.h"
#include "hdyolo_spatial.h"

namespace {

struct Grid { int cell, ncx, ncy, ncells; };

// the cell of a point, ncells for an absent one (which ranks behind every cell)
__device__ __forceinline__ int cell_of(const i32x4& p, const Grid& g) {
    if (p.x < 0 || p.y < 0) return g.ncells;
    const int cx = min(p.x / g.cell, g.ncx - 1), cy = min(p.y / g.cell, g.ncy - 1);
    return cy * g.ncx + cx;
}

struct Run { int s, e; };

// the points of the cells c0 .. c1 of grid row ry: consecutive cells of a row are one contiguous range [s, e) of pts, from two entries of
// cell_start, clamped into [0, N] (safe on any cell_start)
__device__ __forceinline__ Run cell_run(const int* cell_start, const Grid& g, int N, int ry, int c0, int c1) {
    return {max(cell_start[ry * g.ncx + c0], 0), min(cell_start[ry * g.ncx + c1 + 1], N)};
}

int check_pts(const char* who, const int* pts, long long pts_elems, int N) {
    HDY_ARG(N >= 0 && pts_elems >= 0, "%s: negative count (N=%d, pts_elems=%lld)", who, N, pts_elems);
    HDY_ARG(pts_elems == 4ll * N, "%s: pts_elems=%lld, the call reads 4 * N = 4 * %d", who, pts_elems, N);
    HDY_ARG(N == 0 || pts, "%s: null pts pointer", who);
    HDY_ARG(((uintptr_t)pts & 15) == 0, "%s: misaligned pts pointer (16 bytes)", who);
    return HDY_OK;
}

int check_grid(const char* who, int cell_units, int ncx, int ncy) {
    HDY_ARG(cell_units >= 1, "%s: cell_units=%d must be positive", who, cell_units);
    HDY_ARG(ncx >= 1 && ncy >= 1 && (long long)ncx * ncy <= HDY_SPATIAL_MAX_CELLS, "%s: a grid of %d x %d cells (sides >= 1, at most %d cells)", who,
            ncx, ncy, HDY_SPATIAL_MAX_CELLS);
    return HDY_OK;
}

// verb: "reads" or "writes", what the call does with cell_start
int check_cell_start(const char* who, long long elems, int ncells, const char* verb) {
    HDY_ARG(elems == (long long)ncells + 1, "%s: cell_start_elems=%lld, the call %s ncx * ncy + 1 = %d", who, elems, verb, ncells + 1);
    return HDY_OK;
}

}  // namespace
