// exact_walk.hpp -- the point grid as a search reads it (Grid, GridMeta, a point's cell, a row of cells as one range of sorted
// points in the dense and the sparse layout) and the EXACT walk over it (walk_exact: the searches that return f64 distances).  No HIP
// type: point_grid.hpp includes it for the kernels, and a host test (tests/test_exact_walk_host.py, through
// tests/abi/exact_walk_host.cpp) compiles the same text with the host C++ compiler, builds the cell arrays itself and holds the
// walk -- its answers, what it scans and what it turns away -- to brute force.  Under hipcc every function is inlined into the kernel
// that uses it.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef CWIPC_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_HOST_DEVICE __host__ __device__
#else
#define CWIPC_HOST_DEVICE
#endif
#endif

#ifndef CWIPC_FORCEINLINE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_FORCEINLINE __forceinline__
#else
#define CWIPC_FORCEINLINE inline
#endif
#endif

namespace cwipc_amd {

struct Grid {
    float mn[3];
    int dim[3];
    double h;
    double inv_h;
    int nsegx;   // sparse layout: segments (16 cells along x) per row of cells
};

// Sparse layout of the grid for big clouds.  A surface occupies a percent or two of a fine 3-D grid: clearing and scanning a
// dense array of 10^8 cells costs more than the search saves.  Cells are grouped into SEGMENTS of 16 along x; only
// segments that hold points get cells, numbered in the order of the segments (x fastest), so the cells of a row of the
// grid are still one contiguous run of the sorted points, whatever segments are missing in between.
constexpr int SEG = 16, SEG_SHIFT = 4;

// The dense layout's grid is decided ON THE DEVICE (small and medium clouds: a tile of a frame is filtered in ~0.1 ms, and two
// host round trips -- for the bounding box, for the occupancy census -- were a third of that): the kernels read the grid
// from this block, which two one-wave kernels fill in.
struct GridMeta {
    Grid g;
    double ext[3], maxext;
    uint32_t occ;      // occupied cells of the first count (census)
    uint32_t refine;   // 1: the grid was coarsened after the census, the cells are counted again
};

// (int max / min that the host compiler and hipcc both take)
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE int walk_max(int a, int b) { return a > b ? a : b; }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE int walk_min(int a, int b) { return a < b ? a : b; }

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE int cell_coord(const Grid &g, float v, int a) {
    int c = (int)floor(((double)v - (double)g.mn[a]) * g.inv_h);
    c = c < 0 ? 0 : c;
    return c >= g.dim[a] ? g.dim[a] - 1 : c;
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint32_t cell_of(const Grid &g, float x, float y, float z) {
    return (uint32_t)cell_coord(g, x, 0) + (uint32_t)g.dim[0] * ((uint32_t)cell_coord(g, y, 1) + (uint32_t)g.dim[1] * (uint32_t)cell_coord(g, z, 2));
}

// The slot of a device-decided grid that holds the grid in use, and that grid's counts (the small clouds' flow: the coarser
// grid's slot and counts once it has been decided on; every other flow gives no counts2).
struct GridSlot { const GridMeta *gm; const uint32_t *counts; };
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE GridSlot grid_slot(const GridMeta *gm, const uint32_t *counts, const uint32_t *counts2) {
    if (counts2 && gm[1].refine) { gm += 1; counts = counts2; }
    return GridSlot{gm, counts};
}

// The grid as a search kernel reads it, from the members of a GridView passed as kernel arguments.
template <bool SPARSE>
struct GridRows {
    Grid g;
    const uint32_t *starts, *counts;
    CWIPC_HOST_DEVICE CWIPC_FORCEINLINE GridRows(const Grid &gv, const GridMeta *gm, const uint32_t *starts_, const uint32_t *counts_, const uint32_t *counts2) {
        const GridSlot slot = grid_slot(gm, counts_, counts2);
        g = slot.gm ? slot.gm->g : gv;
        starts = starts_;
        counts = slot.counts;
    }
    // Cells that are neighbours along x are neighbours in `sorted` (the counting sort runs x fastest), so a
    // row of cells x0..x1 is ONE range of points: two index loads per row instead of two per cell.
    CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void range(int x0, int x1, int y, int z, uint32_t &first, uint32_t &last) const {
        if (SPARSE) {
            // the cells of this row that exist, from the first at or after x0 to the last at or before x1: an empty segment's
            // entry names the next segment that exists, whose first cell is where everything before it ends
            const uint32_t rowseg = (uint32_t)g.nsegx * ((uint32_t)y + (uint32_t)g.dim[1] * (uint32_t)z);
            const uint32_t i0 = counts[rowseg + ((uint32_t)x0 >> SEG_SHIFT)], i1 = counts[rowseg + ((uint32_t)x1 >> SEG_SHIFT)];
            first = starts[((i0 >> 1) << SEG_SHIFT) + ((i0 & 1u) ? ((uint32_t)x0 & (SEG - 1)) : 0u)];
            last = starts[((i1 >> 1) << SEG_SHIFT) + ((i1 & 1u) ? ((uint32_t)x1 & (SEG - 1)) + 1u : 0u)];
            return;
        }
        const uint32_t base = (uint32_t)g.dim[0] * ((uint32_t)y + (uint32_t)g.dim[1] * (uint32_t)z);
        const uint32_t c1 = base + (uint32_t)x1;
        first = starts[base + (uint32_t)x0];
        last = starts[c1] + counts[c1];
    }
};

// The EXACT walk: every cell that can hold a point under limit(), in growing cubic shells around cell c (the query q's cell,
// clamped to the grid), wherever q lies.  The searches that return f64 distances use it: nn_distance2_kernel and nn_jobs_kernel
// (kernels_nn.hip) and icp_correspond_kernel (kernels_icp.hip); so the three walk the same cells and turn away the same ones.
//   limit()            what a candidate has to stay under, read again at every test: the scans in between lower it
//   scan(first, last)  the caller's look at sorted[first, last)
// The lower bounds on the distance to what has not been looked at -- the box as a whole, a row of cells, an end cell, everything
// beyond shell r -- come from the cells' faces in f64, the query's distance to the box included when it lies outside, each taken
// short by 1e-9 of itself and 1e-6 of a cell (a point's cell is floor((v - mn) / h) in f64: it may sit a rounding error beyond its
// cell's face, some 1e-13 of a cell).  The walk ends when the bound of everything beyond the shell has reached limit(), or the
// shells have covered the grid: a query far from every point with no limit scans the whole grid.
//   EVERY BOUND IS SHORT, and a row, an end cell or a shell is turned away only when its bound is >= limit().  The bound of cells
//   that hold a point at distance d is strictly below d * d (short by 1e-9 of itself; where that leaves nothing it is 0, and a
//   limit of 0 has all its equals in the cell the search begins with: they have the query's own coordinates).  So a cell that
//   holds a point AT limit() is never turned away, whatever order the cells are visited in: a scan that breaks ties among equally
//   distant candidates (the correspondences' smallest original index) sees all of them, and its answer is a value, not an accident
//   of the counting sort.  A bound only ever turns away cells that cannot hold an answer, so no result depends on it.  Keep the
//   bounds short when this walk is changed.
template <bool SPARSE, class Limit, class Scan>
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void walk_exact(const GridRows<SPARSE> &rows, const double (&q)[3], const int (&c)[3], Limit &&limit, Scan &&scan) {
    const Grid &g = rows.g;
    // a distance along axis a that no point of the cells on the far side of `face` undercuts, taken short
    auto shorten = [&](double d) {
        const double t = d * (1.0 - 1e-9) - 1e-6 * g.h;
        return t > 0.0 ? t : 0.0;
    };
    // ... to the cells `o` cells away from `cell` (o != 0)
    auto face_gap = [&](int a, int cell, int o) {
        const double face = (double)g.mn[a] + (double)(o < 0 ? cell + o + 1 : cell + o) * g.h;
        return shorten(o < 0 ? q[a] - face : face - q[a]);
    };
    // ... to the grid's box: 0 for a query between its faces
    double box[3], box2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        box[a] = fmax(face_gap(a, -1, 1), face_gap(a, g.dim[a], -1));
        box2 += box[a] * box[a];
    }
    const int maxring = walk_max(walk_max(walk_max(c[0], g.dim[0] - 1 - c[0]), walk_max(c[1], g.dim[1] - 1 - c[1])), walk_max(c[2], g.dim[2] - 1 - c[2]));
    if (box2 < limit()) {   // (a query further from the box than the limit has no answer)
        for (int ring = 0; ring <= maxring; ring++) {
            const int x0 = walk_max(c[0] - ring, 0), x1 = walk_min(c[0] + ring, g.dim[0] - 1);
            const double gx_lo = c[0] - ring >= 0 && ring > 0 ? face_gap(0, c[0], -ring) : 0.0;
            const double gx_hi = c[0] + ring < g.dim[0] && ring > 0 ? face_gap(0, c[0], ring) : 0.0;
            for (int dz = -ring; dz <= ring; dz++) {
                const int z = c[2] + dz;
                if (z < 0 || z >= g.dim[2]) continue;
                const double gz = dz == 0 ? box[2] : face_gap(2, c[2], dz);
                for (int dy = -ring; dy <= ring; dy++) {
                    const int y = c[1] + dy;
                    if (y < 0 || y >= g.dim[1]) continue;
                    const double gy = dy == 0 ? box[1] : face_gap(1, c[1], dy);
                    const double gyz = gy * gy + gz * gz;
                    if (gyz >= limit()) continue;
                    const bool face = dz == -ring || dz == ring || dy == -ring || dy == ring;
                    uint32_t first, last;
                    if (face) {   // the whole row belongs to the shell
                        rows.range(x0, x1, y, z, first, last);
                        scan(first, last);
                    } else {      // only its two end cells do
                        if (c[0] - ring >= 0 && gyz + gx_lo * gx_lo < limit()) {
                            rows.range(c[0] - ring, c[0] - ring, y, z, first, last);
                            scan(first, last);
                        }
                        if (c[0] + ring < g.dim[0] && gyz + gx_hi * gx_hi < limit()) {
                            rows.range(c[0] + ring, c[0] + ring, y, z, first, last);
                            scan(first, last);
                        }
                    }
                }
            }
            // everything not looked at yet lies at least one more cell away along some axis
            double beyond = INFINITY;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (c[a] - ring - 1 >= 0) beyond = fmin(beyond, face_gap(a, c[a], -(ring + 1)));
                if (c[a] + ring + 1 < g.dim[a]) beyond = fmin(beyond, face_gap(a, c[a], ring + 1));
            }
            if (!(limit() > beyond * beyond)) break;
        }
    }
}

}  // namespace cwipc_amd
