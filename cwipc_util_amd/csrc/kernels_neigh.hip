// kernels_neigh.hip -- gfx950 kernels of cwipc_hip_radius_counts, cwipc_hip_radius_outlier_filter and cwipc_hip_smooth: what a point's
// fixed-radius neighbourhood says about it (RULE N of include/cwipc_util_amd/hip_ext.h has the contract in full;
// tests/neigh_model.py is its numpy and scipy model).
//
//   count    one lane per point of the point grid's sorted array (grid_and_search, any of its three flows).  walk_exact with the
//            constant limit r2 is an exact fixed-radius search, as for the clusters' link kernel (kernels_cluster.hip): every
//            candidate with d2 < r2 (RULE K's f64 arithmetic, strictly) and, under SAME_TILE, the lane's tile byte is counted in a
//            register, the lane's own point among them; count - 1 goes to the point's ORIGINAL index, 0 for a non-finite point.
//   keep     drop[i] = 0 (keep) or 1: the float plane that the outlier filter's stable compaction takes (sor_select), exactly as
//            cluster_keep feeds it.
//   smooth   the same walk; per neighbour the quantised offset and the biweight of smooth_terms.hpp go into ten 64-bit integer sums
//            in registers (W, S1[3], S2[6]) and a count.  Integer sums do not depend on the order of the candidates, so neither the
//            grid's layout nor the order of points in a cell reaches the result.  Behind the walk the same lane decides whether the
//            point moves, solves for the normal (smallest_eigvec.hpp) and stores three floats at the original index; a point that
//            does not move gets the input's words, bit for bit.
// The products in the sums are 32 x 32 -> 64 bit (|o| <= 2^16, w <= 2^12, w * o <= 2^28): one v_mad_i64_i32 each, nine per
// neighbour, no full 64-bit multiply.  The solve stays in the walk's kernel: a second kernel would have to carry eleven 64-bit words
// per point through memory for a solve whose lanes differ only in how many Jacobi sweeps they need (three to five of twelve).
#include "point_grid.hpp"
#include "smooth_terms.hpp"

namespace cwipc_amd {

namespace {

constexpr int NEIGH_GRID_WIDTH = 15;   // the grid's cell size: the cluster filter's (about eight points to an occupied cell)

struct CountArgs {
    const uint32_t *rgbt;   // the cloud's colour / tile words, original order
    uint32_t *counts;       // n words, original order
    double r2;
    int same_tile;
};

template <bool SPARSE>
__global__ void __launch_bounds__(QB) neigh_count_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted, size_t n,
                                                        const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count,
                                                        const uint32_t *__restrict__ cell_count2, CountArgs A) {
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    if (qi >= n) return;
    const float4 me = sorted[qi];
    const uint32_t i = __float_as_uint(me.w);
    uint32_t count = 0;
    if (isfinite(me.x) && isfinite(me.y) && isfinite(me.z)) {
        const double q[3] = {(double)me.x, (double)me.y, (double)me.z};
        const int c[3] = {cell_coord(g, me.x, 0), cell_coord(g, me.y, 1), cell_coord(g, me.z, 2)};
        const uint32_t tile_i = A.same_tile ? A.rgbt[i] >> 24 : 0u;
        auto limit = [&]() { return A.r2; };
        auto candidate = [&](const float4 p) {
            const double dx = (double)p.x - q[0], dy = (double)p.y - q[1], dz = (double)p.z - q[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 < A.r2)) return;   // (a candidate with a non-finite coordinate: inf or NaN, never under the limit)
            if (A.same_tile && (A.rgbt[__float_as_uint(p.w)] >> 24) != tile_i) return;
            count++;
        };
        auto scan = [&](uint32_t first, uint32_t last) { scan_range<1>(sorted, first, last, candidate); };
        walk_exact(rows, q, c, limit, scan);
        if (count) count--;   // the point itself (r2 == 0 finds nobody, not even it)
    }
    A.counts[i] = count;
}

__global__ void __launch_bounds__(GRID_BLK) neigh_keep_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                             const uint32_t *__restrict__ counts, size_t n, unsigned long long min_neighbours,
                                                             float *__restrict__ drop) {
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) {
        const bool keep = isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i]) && (unsigned long long)counts[i] >= min_neighbours;
        drop[i] = keep ? 0.f : 1.f;
    }
}

struct SmoothArgs {
    const uint32_t *in[3];   // the input's coordinate planes as words: what a point that does not move gets
    const uint32_t *rgbt;    // the cloud's colour / tile words, original order
    float *out[3];           // the result's coordinate planes
    double r2, s;            // radius * radius, 65536 / radius
    int same_tile;
    uint32_t min_neighbours;
};

template <bool SPARSE>
__global__ void __launch_bounds__(QB) neigh_smooth_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted, size_t n,
                                                         const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count,
                                                         const uint32_t *__restrict__ cell_count2, SmoothArgs A) {
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    if (qi >= n) return;
    const float4 me = sorted[qi];
    const uint32_t i = __float_as_uint(me.w);
    bool moved = false;
    double disp[3] = {0.0, 0.0, 0.0};
    if (isfinite(me.x) && isfinite(me.y) && isfinite(me.z)) {
        const double q[3] = {(double)me.x, (double)me.y, (double)me.z};
        const int c[3] = {cell_coord(g, me.x, 0), cell_coord(g, me.y, 1), cell_coord(g, me.z, 2)};
        const uint32_t tile_i = A.same_tile ? A.rgbt[i] >> 24 : 0u;
        SmoothSums S;
        auto limit = [&]() { return A.r2; };
        // (always_inline on the lambdas that touch the sums, as in the direction filter: behind a call they would go to scratch memory)
        auto candidate = [&](const float4 p) __attribute__((always_inline)) {
            const double d[3] = {(double)p.x - q[0], (double)p.y - q[1], (double)p.z - q[2]};
            const double d2 = smooth_d2(d);
            if (!(d2 < A.r2)) return;
            if (A.same_tile && (A.rgbt[__float_as_uint(p.w)] >> 24) != tile_i) return;
            smooth_add(S, d, d2, A.r2, A.s);
        };
        auto scan = [&](uint32_t first, uint32_t last) __attribute__((always_inline)) { scan_range<1>(sorted, first, last, candidate); };
        walk_exact(rows, q, c, limit, scan);
        moved = smooth_moves(S.cnt, A.min_neighbours);
        if (moved) smooth_displacement(S, A.s, disp);
    }
    if (moved) {
        A.out[0][i] = (float)((double)me.x + disp[0]);
        A.out[1][i] = (float)((double)me.y + disp[1]);
        A.out[2][i] = (float)((double)me.z + disp[2]);
    } else {
        uint32_t *const ow[3] = {reinterpret_cast<uint32_t *>(A.out[0]), reinterpret_cast<uint32_t *>(A.out[1]), reinterpret_cast<uint32_t *>(A.out[2])};
        for (int a = 0; a < 3; a++) ow[a][i] = A.in[a][i];
    }
}

}  // namespace

bool neigh_counts(const DeviceSoA &src, double r2, bool same_tile, uint32_t *counts) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (src.npoints == 0 || !counts) return false;
    CountArgs A{};
    A.rgbt = src.rgbt();
    A.counts = counts;
    A.r2 = r2;
    A.same_tile = same_tile ? 1 : 0;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        const unsigned qgrid = (unsigned)((v.n + QB - 1) / QB);
        if (v.sparse)
            CW_LAUNCH("neigh_count", (neigh_count_kernel<true>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, A);
        else
            CW_LAUNCH("neigh_count", (neigh_count_kernel<false>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, A);
        return hipGetLastError() == hipSuccess;
    };
    return grid_and_search(src, NEIGH_GRID_WIDTH, true, search);
}

bool neigh_keep_flags(const DeviceSoA &src, const uint32_t *counts, uint64_t min_neighbours, float *drop) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t n = src.npoints;
    if (n == 0 || !counts || !drop) return false;
    CW_LAUNCH("neigh_keep", neigh_keep_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, src.x(), src.y(), src.z(), counts, n,
              (unsigned long long)min_neighbours, drop);
    return hipGetLastError() == hipSuccess;
}

bool neigh_smooth(const DeviceSoA &src, double radius, bool same_tile, uint32_t min_neighbours, const DeviceSoA &dst) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (src.npoints == 0 || dst.npoints != src.npoints || !smooth_radius_ok(radius)) return false;
    SmoothArgs A{};
    A.in[0] = reinterpret_cast<const uint32_t *>(src.x());
    A.in[1] = reinterpret_cast<const uint32_t *>(src.y());
    A.in[2] = reinterpret_cast<const uint32_t *>(src.z());
    A.rgbt = src.rgbt();
    A.out[0] = dst.x();
    A.out[1] = dst.y();
    A.out[2] = dst.z();
    A.r2 = radius * radius;
    A.s = SMOOTH_FIX / radius;
    A.same_tile = same_tile ? 1 : 0;
    A.min_neighbours = min_neighbours;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        const unsigned qgrid = (unsigned)((v.n + QB - 1) / QB);
        if (v.sparse)
            CW_LAUNCH("neigh_smooth", (neigh_smooth_kernel<true>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, A);
        else
            CW_LAUNCH("neigh_smooth", (neigh_smooth_kernel<false>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, A);
        return hipGetLastError() == hipSuccess;
    };
    return grid_and_search(src, NEIGH_GRID_WIDTH, true, search);
}

}  // namespace cwipc_amd
