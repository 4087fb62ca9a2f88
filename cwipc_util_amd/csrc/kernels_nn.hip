// kernels_nn.hip -- nearest distances from one cloud to another on gfx950 (the registration analyzer).
//
// Reference: python/cwipc/registration/analyze.py:120-123, scipy.spatial.KDTree.query(points, k=[nth + 1], distance_upper_bound=max):
// per SOURCE point the distance to its (nth + 1)-th nearest REFERENCE point, inf when fewer than nth + 1 lie closer than max.
// Here the squared distance, in f64: d2 = (dx*dx + dy*dy) + dz*dz with dx = (double)qx - (double)px, every operation rounded on
// its own (-ffp-contract=off) -- what scipy's tree holds before its final sqrt, bit for bit; the caller takes the root on the host.
//
// The grid is the point grid built over the reference cloud (grid_and_search, any of its three flows); the queries are the
// points of another cloud, one lane each, in the caller's order, wherever they lie:
//   * the search starts from the query's cell CLAMPED to the grid and walks growing cubic shells of cells around it;
//   * the candidate list is kept in f64 (KCAP = 2, 4 or 32 sorted registers), so the selection is made on the very values that are
//     returned -- an fp32 search with a margin and a second pass would read every candidate's coordinates twice to save registers
//     that this kernel has to spare (at the tooling's nth of 0 or 1 the list is two registers pairs);
//   * lower bounds on the distance to what has not been looked at -- the box as a whole, a row of cells, everything beyond shell r --
//     come from the cells' faces in f64, the query's distance to the box included when it lies outside, each taken short by
//     1e-9 of itself and 1e-6 of a cell (a point's cell is floor((v - mn) / h) in f64: it may sit a rounding error beyond its cell's
//     face, some 1e-13 of a cell); a bound only ever turns away cells that cannot hold an answer, so the result does not depend on it;
//   * the search ends when the bound has passed the (nth + 1)-th candidate or max_distance, or the shells have covered the grid.  A
//     query far from every reference point with no max_distance therefore scans the whole grid: correct, and as slow as it sounds.
// A distance is a value: which of two equally distant points is kept, and the order the counting sort left a cell's points in,
// cannot change it -- two calls give the same bits.
#include "point_grid.hpp"

#include <algorithm>

namespace cwipc_amd {

namespace {

constexpr int NN_GRID_WIDTH = 15;

struct NNArgs {
    const float *qx, *qy, *qz;   // the source cloud's planes
    size_t nq;
    int want;                    // nth + 1
    double max2;                 // max_distance^2 in f64 (inf: no bound); candidates must be strictly below
    double *out;                 // nq squared distances, the caller's order
};

__global__ void __launch_bounds__(GRID_BLK) nn_fill_inf_kernel(double *__restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) out[i] = INFINITY;
}

template <int KCAP, bool SPARSE>
__global__ void __launch_bounds__(QB) nn_distance2_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted,
                                                         const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count,
                                                         const uint32_t *__restrict__ cell_count2, NNArgs A) {
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    if (qi >= A.nq) return;
    const float qf[3] = {A.qx[qi], A.qy[qi], A.qz[qi]};
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    const int c[3] = {cell_coord(g, qf[0], 0), cell_coord(g, qf[1], 1), cell_coord(g, qf[2], 2)};
    const int pad = KCAP - A.want;
    double best[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; j++) best[j] = j < pad ? -INFINITY : INFINITY;
    // what a candidate has to stay under: the (nth + 1)-th distance so far and the caller's bound
    auto limit = [&]() { return fmin(best[KCAP - 1], A.max2); };
    auto candidate = [&](const float4 p) {
        const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < limit()) {
            // sorted insert, the largest drops out; top down, every slot from old values
#pragma unroll
            for (int j = KCAP - 1; j >= 1; j--) best[j] = d2 < best[j - 1] ? best[j - 1] : fmin(best[j], d2);
            best[0] = fmin(best[0], d2);
        }
    };
    auto scan = [&](uint32_t first, uint32_t last) { scan_range<1>(sorted, first, last, candidate); };
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
    if (box2 < limit()) {   // (a query further from the box than max_distance has no answer)
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
    A.out[qi] = best[KCAP - 1];
}

template <int KCAP>
void launch_nn(const GridView &v, const NNArgs &A, hipStream_t s) {
    const unsigned qgrid = (unsigned)((A.nq + QB - 1) / QB);
    if (v.sparse)
        CW_LAUNCH("nn_distance2", (nn_distance2_kernel<KCAP, true>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.starts, v.counts, v.counts2, A);
    else
        CW_LAUNCH("nn_distance2", (nn_distance2_kernel<KCAP, false>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.starts, v.counts, v.counts2, A);
}

}  // namespace

bool nn_distance2(const DeviceSoA &source, const DeviceSoA &reference, int nth, double max_distance, double *dev_out) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t nq = source.npoints;
    if (nq == 0) return true;
    if (nth < 0 || nth >= NN_MAX_NTH + 1 || !(max_distance > 0.0)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_nn_distance2", "nth must lie between 0 and 31, max_distance must be positive (inf: no bound)");
        return false;
    }
    if (reference.npoints == 0) {
        CW_LAUNCH("nn_fill_inf", nn_fill_inf_kernel, dim3(grid_blocks(nq)), dim3(GRID_BLK), 0, c.stream, dev_out, nq);
        return hipGetLastError() == hipSuccess;
    }
    NNArgs A{};
    A.qx = source.x(); A.qy = source.y(); A.qz = source.z();
    A.nq = nq;
    A.want = nth + 1;
    A.max2 = max_distance * max_distance;
    A.out = dev_out;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        if (A.want <= 2) launch_nn<2>(v, A, s);
        else if (A.want <= 4) launch_nn<4>(v, A, s);
        else launch_nn<32>(v, A, s);
        return hipGetLastError() == hipSuccess;
    };
    // The grid's cell size: as for the outlier filter's k-NN of width 15 (about eight points to an occupied cell), of nth + 1 beyond.
    // The self-search's own choice for nth + 1 = 1 or 2 is a point or two per cell, right for queries that ARE reference points;
    // a query of another cloud may lie many cells from the nearest reference point (two camera tiles overlap along a seam
    // only), and until its first candidate turns up nothing bounds the shells it walks: (2r + 1)^2 rows of cells for shell r.
    // Cells 2.8 times as wide make that walk some twenty times shorter and give a near query a few dozen candidates more.
    return grid_and_search(reference, std::max(nth + 1, NN_GRID_WIDTH), true, search);
}

}  // namespace cwipc_amd
