// point_grid.hpp -- the uniform grid over a cloud's points, and what a search kernel needs to walk it.
//
// kernels_grid.hip builds the grid (grid_and_search: a counting sort of the points into cells, three flows) and calls the
// client's search on it; the clients are the outlier filter's k-NN (kernels_sor.hip), the direction filter's normals
// (kernels_direction.hip), the registration analyzer's cross-cloud distances (kernels_nn.hip) and the ICP correspondences
// (kernels_icp.hip).  The device helpers below are
// the parts of a shell search that those kernels share: which slot of a device-decided grid to read, a row of cells as one range
// of sorted points, the candidate scan, FLANN's fp32 distance, the sorted register list, the bounds that turn rows away, the
// walk over a shell of cells (walk_shell: the fp32 k-NN searches) and the whole exact walk of the searches that return f64
// distances (walk_exact).  All of them are inlined into the kernel that uses them.
#pragma once

#include "internal.hpp"

#include <cfloat>
#include <cmath>
#include <functional>

namespace cwipc_amd {

constexpr int GRID_BLK = 256;   // threads per workgroup of the per-point kernels around the grid
static inline unsigned grid_blocks(size_t n) {
    size_t g = (n + GRID_BLK - 1) / GRID_BLK;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    return (unsigned)g;
}

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

// What grid_and_search hands to a search: the points in cell order (x, y, z, original index; cells run x fastest) and the
// per-cell arrays of the layout the flow has built.  The search is launched on the stream it is given, where the flows would
// launch the outlier filter's k-NN; the flow frees the grid's arrays behind it.
//   gm       the device-decided grid (dense layout), or nullptr and g (sparse layout: the host decided)
//   counts2  small clouds' flow only: gm has two slots, and slot 1 with counts2 holds the coarser grid when gm[1].refine is set
//            -- a kernel cannot know before it runs, so it takes all of gm, counts, counts2 and asks grid_slot / GridRows
//   sparse   counts is the segment table (seg_pack_kernel), starts is indexed by the cells that exist (one entry more: the end);
//            otherwise starts / counts are indexed by cell
struct GridView {
    Grid g;
    const GridMeta *gm;
    const float4 *sorted;
    size_t n;
    const uint32_t *starts, *counts, *counts2;
    bool sparse;
};
// launches the search's kernels; false: the search failed
typedef std::function<bool(const GridView &, hipStream_t)> GridSearch;

// The grid over src (three flows: small clouds, the dense layout decided on the device, the sparse layout) and the search on it.
// k sets the cell size: that of the outlier filter's k-NN of this width (an occupied cell holds a fraction of k + 1 points).
// all_layouts: the search reads every GridView; false: only the dense layout without counts2 (the medium clouds' flow, any size).
// No wait behind the search.  An empty cloud: true, the search is not called.
bool grid_and_search(const DeviceSoA &src, int k, bool all_layouts, const GridSearch &search);

// One lane per query, 128 queries per workgroup: the launch shape of the search kernels.
constexpr int QB = 128;

__device__ __forceinline__ int cell_coord(const Grid &g, float v, int a) {
    int c = (int)floor(((double)v - (double)g.mn[a]) * g.inv_h);
    c = c < 0 ? 0 : c;
    return c >= g.dim[a] ? g.dim[a] - 1 : c;
}

__device__ __forceinline__ uint32_t cell_of(const Grid &g, float x, float y, float z) {
    return (uint32_t)cell_coord(g, x, 0) + (uint32_t)g.dim[0] * ((uint32_t)cell_coord(g, y, 1) + (uint32_t)g.dim[1] * (uint32_t)cell_coord(g, z, 2));
}

// The slot of a device-decided grid that holds the grid in use, and that grid's counts (the small clouds' flow: the coarser
// grid's slot and counts once it has been decided on; every other flow gives no counts2).
struct GridSlot { const GridMeta *gm; const uint32_t *counts; };
__device__ __forceinline__ GridSlot grid_slot(const GridMeta *gm, const uint32_t *counts, const uint32_t *counts2) {
    if (counts2 && gm[1].refine) { gm += 1; counts = counts2; }
    return GridSlot{gm, counts};
}

// The grid as a search kernel reads it, from the members of a GridView passed as kernel arguments.
template <bool SPARSE>
struct GridRows {
    Grid g;
    const uint32_t *starts, *counts;
    __device__ __forceinline__ GridRows(const Grid &gv, const GridMeta *gm, const uint32_t *starts_, const uint32_t *counts_, const uint32_t *counts2) {
        const GridSlot slot = grid_slot(gm, counts_, counts2);
        g = slot.gm ? slot.gm->g : gv;
        starts = starts_;
        counts = slot.counts;
    }
    // Cells that are neighbours along x are neighbours in `sorted` (the counting sort runs x fastest), so a
    // row of cells x0..x1 is ONE range of points: two index loads per row instead of two per cell.
    __device__ __forceinline__ void range(int x0, int x1, int y, int z, uint32_t &first, uint32_t &last) const {
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

// take(p) for every STRIDE-th point of sorted[first, last), four loads in flight at a time (the loop is latency-bound
// otherwise: one dependent 16-byte load per lane and iteration)
template <uint32_t STRIDE, class Take>
__device__ __forceinline__ void scan_range(const float4 *__restrict__ sorted, uint32_t first, uint32_t last, Take &&take) {
    uint32_t e = first;
    for (; e + 3 * STRIDE + 1 <= last; e += 4 * STRIDE) {
        const float4 p0 = sorted[e], p1 = sorted[e + STRIDE], p2 = sorted[e + 2 * STRIDE], p3 = sorted[e + 3 * STRIDE];
        take(p0); take(p1); take(p2); take(p3);
    }
    for (; e < last; e += STRIDE) take(sorted[e]);
}

// FLANN L2_Simple<float>: separately rounded fp32 operations, (dx*dx + dy*dy) + dz*dz -- x and y as one packed subtraction
// and one packed multiplication: the same operations, summed in the same order
__device__ __forceinline__ float flann_dist2(const float4 &q, const float4 &p) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 dxy = f32x2{q.x, q.y} - f32x2{p.x, p.y};
    const f32x2 sq = dxy * dxy;
    const float dz = __fsub_rn(q.z, p.z);
    return __fadd_rn(__fadd_rn(sq.x, sq.y), __fmul_rn(dz, dz));
}

// Insert into an ascending list in registers, the largest value drops out: the new j-th smallest is the MEDIAN of the old
// (j-1)-th, the old j-th and the newcomer -- one v_med3_f32 per slot, all from old values (top down, in place), no chain of
// dependent min / max pairs.  Unused leading slots hold -inf, so the largest kept value is always the last register.
template <int KCAP>
__device__ __forceinline__ void sorted_insert(float (&best)[KCAP], float v) {
#pragma unroll
    for (int j = KCAP - 1; j >= 1; j--) best[j] = __builtin_amdgcn_fmed3f(best[j - 1], best[j], v);
    best[0] = fminf(best[0], v);
}

// Shell `ring` of cells around a query proves a list complete once its worst kept distance is under ring * h: every point not
// yet seen lies beyond that
__device__ __forceinline__ bool shell_proves(const Grid &g, int ring, float worst) {
    const double reach = (double)ring * g.h;
    return (double)worst < reach * reach * (1.0 - 1e-6);
}

// Ring 1's bound for a row of cells: the squared distance along one axis from v to the cells `o` (-1, 0, 1) away from the
// query's cell, whose lower face is lo_face -- in fp32, taken short by eps = 1e-5 h: rounding never skips a row that matters
__device__ __forceinline__ float near_gap(float v, float lo_face, float hf, float eps, int o) {
    const float d = o == 0 ? 0.f : (o < 0 ? v - lo_face : lo_face + hf - v);
    const float t = fmaxf(d - eps, 0.f);
    return t * t;
}

// Shells beyond the first: the squared distance along axis a from v to the cells `o` cells away from `cell`, from the cells'
// faces in f64 (the cell of a point is floor((v - mn) / h) in f64 too).  The margin goes in once, in f64, before the value is
// rounded to fp32: what is added up in fp32 stays under the true distance by more than the three roundings of the candidates'
// own fp32 distances.
__device__ __forceinline__ float shell_gap2(const Grid &g, float v, int a, int cell, int o) {
    if (o == 0) return 0.f;
    const double face = (double)g.mn[a] + (double)(o < 0 ? cell + o + 1 : cell + o) * g.h;
    const double d = o < 0 ? (double)v - face : face - (double)v;
    return d > 0.0 ? (float)(d * d * (1.0 - 1e-6)) : 0.f;
}

// The walk over shell `ring` >= 2 around the query q in cell (cx, cy, cz): scan(first, last) for the face rows whole and for the
// two end cells of the inner rows.  (r4) These shells are for the queries at a cloud's edge, a few lanes of every wave, and the
// whole wave waits for them: a row (or an end cell) is looked up only if it can still hold an answer, its squared distance from
// the query (shell_gap2) not beyond bound() -- `strict`: only strictly beyond is turned away, for a scan that takes candidates AT
// the bound too.  Without the test a lane in ring 2 walked through 34 dependent pairs of loads (row index, candidates), most of
// them for cells on the far side.  bound() is read again for every row: the scans in between lower it.
template <bool SPARSE, class Bound, class Scan>
__device__ __forceinline__ void walk_shell(const GridRows<SPARSE> &rows, const float4 &q, int cx, int cy, int cz, int ring, Bound &&bound, bool strict,
                                           Scan &&scan) {
    const Grid &g = rows.g;
    auto beyond = [&](float gap) { return strict ? gap > bound() : gap >= bound(); };
    const int x0 = max(cx - ring, 0), x1 = min(cx + ring, g.dim[0] - 1);
    const float gx_lo = shell_gap2(g, q.x, 0, cx, -ring), gx_hi = shell_gap2(g, q.x, 0, cx, ring);
    for (int dz = -ring; dz <= ring; dz++) {
        const int z = cz + dz;
        if (z < 0 || z >= g.dim[2]) continue;
        const float gz = shell_gap2(g, q.z, 2, cz, dz);
        for (int dy = -ring; dy <= ring; dy++) {
            const int y = cy + dy;
            if (y < 0 || y >= g.dim[1]) continue;
            const float gyz = gz + shell_gap2(g, q.y, 1, cy, dy);
            if (beyond(gyz)) continue;
            const bool face = dz == -ring || dz == ring || dy == -ring || dy == ring;
            uint32_t first, last;
            if (face) {   // the whole row belongs to the shell
                rows.range(x0, x1, y, z, first, last);
                scan(first, last);
            } else {      // only its two end cells do
                if (cx - ring >= 0 && !beyond(gyz + gx_lo)) { rows.range(cx - ring, cx - ring, y, z, first, last); scan(first, last); }
                if (cx + ring < g.dim[0] && !beyond(gyz + gx_hi)) { rows.range(cx + ring, cx + ring, y, z, first, last); scan(first, last); }
            }
        }
    }
}

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
__device__ __forceinline__ void walk_exact(const GridRows<SPARSE> &rows, const double (&q)[3], const int (&c)[3], Limit &&limit, Scan &&scan) {
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
    const int maxring = max(max(max(c[0], g.dim[0] - 1 - c[0]), max(c[1], g.dim[1] - 1 - c[1])), max(c[2], g.dim[2] - 1 - c[2]));
    if (box2 < limit()) {   // (a query further from the box than the limit has no answer)
        for (int ring = 0; ring <= maxring; ring++) {
            const int x0 = max(c[0] - ring, 0), x1 = min(c[0] + ring, g.dim[0] - 1);
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
