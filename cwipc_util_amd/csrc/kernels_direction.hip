// kernels_direction.hip -- the direction filter on gfx950.
//
// A normal per point, oriented away from the centroid; the point is kept when the normal faces a direction.
// Reference: cwipc_direction_filter (python/cwipc/registration/util.py:114-143), whose normals come from open3d's EstimateNormals
// with KDTreeSearchParamHybrid(radius, max_nn) and orient_normals_towards_camera_location(centroid), then are negated.
//   N(p)   = the points q with |q - p| < radius, the max_nn nearest of them (p itself included, at distance 0)
//   n_raw  = (0, 0, 1) if |N| < 3 or the covariance of N is 0, else the unit eigenvector of its smallest eigenvalue
//   n      = -(n_raw, negated if n_raw . (c - p) < 0),  c = the cloud's centroid (f64 sum)
//   keep p iff n . d >= threshold  (d: the direction, unit length unless it is 0)
// The neighbourhood comes from the point grid (grid_and_search) and the shell search of point_grid.hpp in two passes over the same rows:
// pass 1 keeps the max_nn smallest fp32 distances (the list in registers, its empty slots holding radius^2, so nothing at or beyond
// the radius enters and the shell loop's exit test also ends the search once the shells reach the radius); its last slot is the
// cutoff.  Pass 2 visits the same rows again and sums, for every point at or under the cutoff (all of a tie at the cutoff: the
// result does not depend on the order of the points in a cell), count, sum(q - p) and sum((q - p)(q - p)^T) in int64 fixed point
// (2^-20 of the cutoff distance), which no order of the candidates changes: the normals are the same bits run after run.
#include "point_grid.hpp"
#include "block_scan.hpp"
#include "smallest_eigvec.hpp"

#include <algorithm>

namespace cwipc_amd {

namespace {

constexpr double DIR_FIX = 1048576.0;   // fixed-point units per cutoff distance

// centroid: f64 sums over contiguous slices (fixed order for the fixed launch shape), then the pairwise tree of stats_final_kernel (kernels_sor.hip)
constexpr int CEN_BLOCKS = 1024;
__global__ void __launch_bounds__(GRID_BLK) centroid_partial_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                              double *__restrict__ partial /* [CEN_BLOCKS][3] */) {
    __shared__ double red[3][GRID_BLK / 64];
    double s[3] = {0, 0, 0};
    const size_t per = (n + gridDim.x - 1) / gridDim.x;
    const size_t lo = (size_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    for (size_t i = lo + threadIdx.x; i < hi; i += GRID_BLK) { s[0] += (double)x[i]; s[1] += (double)y[i]; s[2] += (double)z[i]; }
    for (int a = 0; a < 3; a++) {
        k::wave_reduce_sum(s[a]);
        if ((threadIdx.x & 63) == 0) red[a][threadIdx.x >> 6] = s[a];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0;
        for (int w = 0; w < GRID_BLK / 64; w++) t += red[threadIdx.x][w];
        partial[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
    }
}

__global__ void __launch_bounds__(CEN_BLOCKS) centroid_final_kernel(const double *__restrict__ partial, size_t n, double *__restrict__ cen) {
    __shared__ double s[3][CEN_BLOCKS];
    for (int a = 0; a < 3; a++) s[a][threadIdx.x] = partial[threadIdx.x * 3 + a];
    __syncthreads();
    for (unsigned width = CEN_BLOCKS / 2; width >= 1; width >>= 1) {
        double v[3] = {0, 0, 0};
        if (threadIdx.x < width)
            for (int a = 0; a < 3; a++) v[a] = s[a][2 * threadIdx.x] + s[a][2 * threadIdx.x + 1];
        __syncthreads();
        if (threadIdx.x < width)
            for (int a = 0; a < 3; a++) s[a][threadIdx.x] = v[a];
        __syncthreads();
    }
    if (threadIdx.x < 3) cen[threadIdx.x] = s[threadIdx.x][0] / (double)n;
}

struct DirectionArgs {
    float r2;                 // radius^2 in fp32: no candidate at or beyond it is taken
    int want;                 // max_nn
    const double *cen;        // device: the centroid
    double dir[3], threshold;
    float *drop;              // per input point: 0 keep, 1 drop (nullptr: not written)
    float *normals;           // planes x, y, z of `stride` floats each (nullptr: not written)
    size_t stride;
    uint32_t *nn;             // |N(p)| (nullptr: not written)
};

// One lane per point in cell order, as knn_mean_dist_reg_kernel.  KCAP >= want; the first KCAP - want slots hold -inf.
template <int KCAP, bool SPARSE>
__global__ void __launch_bounds__(QB) direction_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted, size_t n,
                                                      const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count,
                                                      const uint32_t *__restrict__ cell_count2, DirectionArgs A) {
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    if (qi >= n) return;
    const float4 q = sorted[qi];
    const int cx = cell_coord(g, q.x, 0), cy = cell_coord(g, q.y, 1), cz = cell_coord(g, q.z, 2);
    const int pad = KCAP - A.want;
    float best[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; j++) best[j] = j < pad ? -INFINITY : A.r2;
    // The rows of shell `ring` (ring 1: shells 0 and 1 together, the query's own row first), a row only if its nearest face is
    // not beyond bound() -- strictly beyond for pass 2, which takes candidates AT the cutoff too.  scan(first, last) takes the points.
    auto visit = [&](int ring, auto bound, bool strict, auto scan) {
        if (ring > 1) { walk_shell(rows, q, cx, cy, cz, ring, bound, strict, scan); return; }
        auto beyond = [&](float gap) { return strict ? gap > bound() : gap >= bound(); };
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
        const float eps = (float)(g.h * 1e-5), hf = (float)g.h;
        const float ylo = (float)((double)g.mn[1] + (double)cy * g.h), zlo = (float)((double)g.mn[2] + (double)cz * g.h);
        constexpr int order[9] = {4, 1, 3, 5, 7, 0, 2, 6, 8};
        auto row = [&](int o) __attribute__((always_inline)) {
            const int r = order[o];
            const int y = cy + (r % 3) - 1, z = cz + (r / 3) - 1;
            if (y < 0 || y >= g.dim[1] || z < 0 || z >= g.dim[2]) return;
            if (o > 0 && beyond(near_gap(q.y, ylo, hf, eps, r % 3 - 1) + near_gap(q.z, zlo, hf, eps, r / 3 - 1))) return;
            uint32_t first, last;
            rows.range(x0, x1, y, z, first, last);
            scan(first, last);
        };
        if (KCAP > 33) {   // the wide lists: unrolled (rolled, max_nn = 64 on a 36 k-point tile takes 16 % longer)
#pragma unroll
            for (int o = 0; o < 9; o++) row(o);
        } else {           // the compiler's choice
            for (int o = 0; o < 9; o++) row(o);
        }
    };
    // pass 1: the want smallest distances under radius^2
    // (always_inline on the lambdas that touch the list and the sums: behind a function call the list goes to scratch memory)
    auto take = [&](const float4 p) __attribute__((always_inline)) {
        const float d2 = flann_dist2(q, p);   // (the outlier filter's fp32 distance)
        if (d2 < best[KCAP - 1]) sorted_insert(best, d2);
    };
    auto scan1 = [&](uint32_t first, uint32_t last) __attribute__((always_inline)) { scan_range<1>(sorted, first, last, take); };
    auto worst = [&]() { return best[KCAP - 1]; };
    const int maxring = max(g.dim[0], max(g.dim[1], g.dim[2]));
    int last_ring = 1;
    for (int ring = 1; ring <= maxring; ring++) {
        visit(ring, worst, false, scan1);
        last_ring = ring;
        // every point not yet seen lies beyond ring * h: the list is final once its last slot (the radius^2 while it is not full) is under that
        if (shell_proves(g, ring, best[KCAP - 1])) break;
    }
    const float cutoff = best[KCAP - 1];
    // pass 2: the moments of the points at or under the cutoff (and under the radius), in fixed point
    const double scale = cutoff > 0.f ? DIR_FIX / sqrt((double)cutoff) : 0.0;
    uint32_t cnt = 0;
    long long s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0};
    auto accumulate = [&](const float4 p) __attribute__((always_inline)) {
        const float d2 = flann_dist2(q, p);
        if (!(d2 <= cutoff && d2 < A.r2)) return;
        cnt++;
        const long long u0 = llrint(((double)p.x - (double)q.x) * scale), u1 = llrint(((double)p.y - (double)q.y) * scale),
                        u2 = llrint(((double)p.z - (double)q.z) * scale);
        s1[0] += u0; s1[1] += u1; s1[2] += u2;
        s2[0] += u0 * u0; s2[1] += u0 * u1; s2[2] += u0 * u2; s2[3] += u1 * u1; s2[4] += u1 * u2; s2[5] += u2 * u2;
    };
    auto scan2 = [&](uint32_t first, uint32_t last) __attribute__((always_inline)) { scan_range<1>(sorted, first, last, accumulate); };
    auto cut = [&]() { return cutoff; };
    for (int ring = 1; ring <= last_ring; ring++) visit(ring, cut, true, scan2);
    // covariance * cnt^2 (the scale does not matter to the eigenvector): cnt * S2 - S1 S1^T
    double nrm[3] = {0.0, 0.0, 1.0};
    if (cnt >= 3) {
        const double m = (double)cnt;
        double a[3][3];
        a[0][0] = m * (double)s2[0] - (double)s1[0] * (double)s1[0];
        a[0][1] = a[1][0] = m * (double)s2[1] - (double)s1[0] * (double)s1[1];
        a[0][2] = a[2][0] = m * (double)s2[2] - (double)s1[0] * (double)s1[2];
        a[1][1] = m * (double)s2[3] - (double)s1[1] * (double)s1[1];
        a[1][2] = a[2][1] = m * (double)s2[4] - (double)s1[1] * (double)s1[2];
        a[2][2] = m * (double)s2[5] - (double)s1[2] * (double)s1[2];
        const bool zero = a[0][0] == 0.0 && a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][1] == 0.0 && a[1][2] == 0.0 && a[2][2] == 0.0;
        if (!zero) smallest_eigvec(a, nrm);
    }
    // towards the centroid, then turned round: away from it
    const double tc = nrm[0] * (A.cen[0] - (double)q.x) + nrm[1] * (A.cen[1] - (double)q.y) + nrm[2] * (A.cen[2] - (double)q.z);
    const double sg = tc < 0.0 ? 1.0 : -1.0;
    for (int a = 0; a < 3; a++) nrm[a] *= sg;
    const double dot = nrm[0] * A.dir[0] + nrm[1] * A.dir[1] + nrm[2] * A.dir[2];
    const uint32_t at = __float_as_uint(q.w);
    if (A.drop) A.drop[at] = dot >= A.threshold ? 0.f : 1.f;
    if (A.normals) {
        A.normals[at] = (float)nrm[0];
        A.normals[A.stride + at] = (float)nrm[1];
        A.normals[2 * A.stride + at] = (float)nrm[2];
    }
    if (A.nn) A.nn[at] = cnt;
}

template <int KCAP>
void launch_direction(const GridView &v, const DirectionArgs &A, hipStream_t s) {
    const unsigned qgrid = (unsigned)((v.n + QB - 1) / QB);
    if (v.sparse)
        CW_LAUNCH("direction_normals", (direction_kernel<KCAP, true>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, A);
    else
        CW_LAUNCH("direction_normals", (direction_kernel<KCAP, false>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, A);
}

}  // namespace

bool direction_normals(const DeviceSoA &src, float radius, int max_nn, const double dir[3], double threshold, float *drop, float *normals,
                       size_t stride, uint32_t *nn_count, double *centroid_dev) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t n = src.npoints;
    if (n == 0) return true;
    if (!(radius > 0.f) || !std::isfinite(radius) || max_nn < 1 || max_nn > DIRECTION_MAX_NN) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_direction_filter", "radius must be positive and finite, max_nn between 1 and 128");
        return false;
    }
    double *partial = (double *)pool_alloc(CEN_BLOCKS * 3 * sizeof(double));
    if (!partial) return false;
    CW_LAUNCH("direction_centroid", centroid_partial_kernel, dim3(CEN_BLOCKS), dim3(GRID_BLK), 0, c.stream, src.x(), src.y(), src.z(), n, partial);
    CW_LAUNCH("direction_centroid", centroid_final_kernel, dim3(1), dim3(CEN_BLOCKS), 0, c.stream, partial, n, centroid_dev);
    c.free_later(partial);
    if (!drop && !normals && !nn_count) return hipGetLastError() == hipSuccess;   // the centroid alone (cwipc_center)
    DirectionArgs A{};
    A.r2 = radius * radius;   // (one fp32 product: -ffp-contract=off)
    A.want = max_nn;
    A.cen = centroid_dev;
    for (int a = 0; a < 3; a++) A.dir[a] = dir[a];
    A.threshold = threshold;
    A.drop = drop;
    A.normals = normals;
    A.stride = stride;
    A.nn = nn_count;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        if (max_nn <= 32) launch_direction<33>(v, A, s);
        else if (max_nn <= 64) launch_direction<65>(v, A, s);
        else launch_direction<129>(v, A, s);
        return hipGetLastError() == hipSuccess;
    };
    // the grid's cell size as for the outlier filter's k-NN of the same width (max_nn points, the query among them); lists wider
    // than that filter's registers hold (33) have only ever run on the medium clouds' dense layout, and stay there
    return grid_and_search(src, std::max(max_nn - 1, 1), max_nn <= 33, search);
}

}  // namespace cwipc_amd
