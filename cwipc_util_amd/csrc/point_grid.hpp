// point_grid.hpp -- the uniform grid over a cloud's points, and what a search kernel needs to walk it.
//
// kernels_grid.hip builds the grid (grid_and_search: a counting sort of the points into cells, three flows) and calls the
// client's search on it; the clients are the outlier filter's k-NN (kernels_sor.hip), the direction filter's normals
// (kernels_direction.hip), the registration analyzer's cross-cloud distances (kernels_nn.hip) and the ICP correspondences
// (kernels_icp.hip).  The device helpers below are
// the parts of a shell search that those kernels share: the candidate scan, FLANN's fp32 distance, the sorted register list, the
// bounds that turn rows away and the walk over a shell of cells (walk_shell: the fp32 k-NN searches).  What needs no HIP type is in
// exact_walk.hpp, included here, so that the host compiler can read it too: the grid itself (Grid, GridMeta, a point's cell),
// which slot of a device-decided grid to read, a row of cells as one range of sorted points (GridRows) and the whole exact walk of
// the searches that return f64 distances (walk_exact).  All of them are inlined into the kernel that uses them.
#pragma once

#include "internal.hpp"
#include "exact_walk.hpp"

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

}  // namespace cwipc_amd
