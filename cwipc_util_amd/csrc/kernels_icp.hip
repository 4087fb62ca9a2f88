// kernels_icp.hip -- point-to-point and point-to-plane ICP on gfx950: correspondences, the sums of a rigid fit and of a plane fit,
// the loops (registration/fine.py and the overlap analyzer of registration/analyze.py).
//
// Reference: python/cwipc/registration/fine.py and analyze.py (OverlapAnalyzer), which call open3d's registration_icp with
// TransformationEstimationPointToPoint and evaluate_registration on the CPU.  Three layers, each with a contract of its own:
//
// Correspondences (icp_correspond_kernel).  One lane per SOURCE point, in the caller's order.  The query is the source point moved
// by the 4x4 matrix T (row-major f64), computed in f64 from the float32 coordinates:
//     px = ((T00*x + T01*y) + T02*z) + T03        (py, pz alike; every operation rounded on its own, -ffp-contract=off)
// and searched in the point grid over the REFERENCE cloud exactly as nn_distance2_kernel (kernels_nn.hip) searches: the query's
// cell is floor((p - mn) * inv_h) of the f64 value, clamped; growing cubic shells; bounds from the cells' faces in f64, each taken
// short by 1e-9 of itself and 1e-6 of a cell.  Per source point: idx = the ORIGINAL index (sorted[].w) of the nearest reference
// point, d2 = (dx*dx + dy*dy) + dz*dz with dx = px - (double)qx; only candidates with d2 < max_distance^2 (strictly) count;
// 0xFFFFFFFF and +inf when there is none, also for a source point with a non-finite coordinate before or after T.  Reference
// points with a non-finite coordinate are not in the grid and are never candidates.
//   AMONG EQUAL d2 THE SMALLEST ORIGINAL INDEX WINS.  The candidate test below says so; what makes it true for candidates in
//   DIFFERENT cells is that every bound is short: a row, an end cell or a shell is turned away only when its bound is >= the best
//   d2 so far, and the bound of cells that hold a point at distance d is strictly below d * d (short by 1e-9 of itself; where that
//   leaves nothing it is 0, and a best d2 of 0 has all its equals in the cell the search begins with: they have the query's own
//   coordinates).  So a cell that holds an equally distant point is never turned away, whatever order the cells are visited in,
//   and idx is a value, not an accident of the counting sort.  Keep the bounds short when this walk is changed.
//
// Fit sums (icp_sums_partial_kernel, icp_sums_final_kernel).  Over the source points that have a correspondence, with pivots cp,
// cq (kernel arguments), a = p - cp (p recomputed as above, not stored) and b = q - cq (q the matched reference point):
//     n | sum a (3) | sum b (3) | sum a b^T (9, row-major: a_i b_j) | sum d2                                  (f64)
// summed the way the KDE kernels sum: the source is cut into chunks of ICP_CHUNK << s points, s the smallest shift that leaves at
// most ICP_MAX_CHUNKS chunks -- a function of the source count alone; one workgroup per chunk, every lane adds its points in
// index order, a fixed shuffle tree closes the wave and lane 0 adds the four waves in order; a second kernel adds the chunks in
// index order and writes the 17 values to the thread's pinned words.  No atomics: two calls give the same bytes.
//
// The loop (icp_point2point) is open3d's registration_icp; it runs inside ONE GridSearch hook, so the grid over the reference is
// built once per run.  T is applied to the ORIGINAL float32 source points on every iteration (open3d moves an f64 copy step by step).
//
// POINT-TO-PLANE (icp_plane_sums_partial_kernel, icp_plane_sums_final_kernel, icp_point2plane).  open3d is not on this stack, so
// nothing is compared with it: this is a restatement of open3d's TransformationEstimationPointToPlane inside registration_icp,
// pinned by a numpy model (tests/icp_plane_model.py).  Correspondences are exactly those above: the same kernel, the same tie
// rule, the same strict bound.  For a matched pair, every operation rounded on its own:
//     p = the moved source point (icp_move),  q = the matched reference point,  m = that reference point's normal
//                                                                               (q and m: (double) of float32)
//     e = p - q,   r = (e0*m0 + e1*m1) + e2*m2
//     c = p x m:   c0 = p1*m2 - p2*m1,  c1 = p2*m0 - p0*m2,  c2 = p0*m1 - p1*m0
//     J = (c0, c1, c2, m0, m1, m2)
// No pivots: this is open3d's form.  The sums, in this order:
//     n | sum J_i J_j for i <= j (21, the upper triangle row-major) | sum J_i r (6) | sum r^2 | sum d2          (f64)
// 29 doubles and n; with the tag 31 of the 32 pinned 64-bit words a thread has.  They are summed by the scheme of the fit sums
// above (the same chunks, four points per lane and step, the same trees), so two calls give the same bytes.  Negating a normal
// negates J and r exactly and leaves every term's bits as they are: the reference's _fix_normal_direction has no effect on this
// aligner and is not ported.
//   The normals are float planes in pool memory (x, y, z, each count(reference) long), gathered by idx like the reference's
// coordinates: direction_normals (kernels_direction.hip) writes them there once per run, before the grid hook -- open3d's
// KDTreeSearchParamHybrid(radius, max_nn) estimate -- or the caller's are copied there.  Only the reference cloud has normals:
// open3d's point-to-plane estimate never reads the source's.
//   The loop (icp_point2plane) is the loop above with the update of plane_fit.hpp: A x = -b with A = sum J J^T, b = sum J r;
// fitness and inlier_rmse come from n and sum d2 (the point distances, not r), and the stop rule is the same.
#include "point_grid.hpp"
#include "rigid_fit.hpp"
#include "plane_fit.hpp"
#include "gicp_terms.hpp"

#include <algorithm>
#include <cstring>

namespace cwipc_amd {

namespace {

constexpr int ICP_GRID_WIDTH = 15;      // the grid's cell size: as for nn_distance2 (kernels_nn.hip)
constexpr uint32_t ICP_NONE = 0xFFFFFFFFu;

struct IcpArgs {
    const float *sx, *sy, *sz;   // the source cloud's planes
    size_t ns;
    double T[12];                // rows 0..2 of the 4x4
    double max2;                 // max_distance^2 in f64 (inf: no bound); candidates must be strictly below
    uint32_t *idx;               // ns original indices of reference points
    double *d2;                  // ns squared distances
};

// the moved point, as the contract states it
__device__ __forceinline__ void icp_move(const double (&T)[12], float x, float y, float z, double (&p)[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) p[r] = ((T[4 * r] * (double)x + T[4 * r + 1] * (double)y) + T[4 * r + 2] * (double)z) + T[4 * r + 3];
}

__global__ void __launch_bounds__(GRID_BLK) icp_fill_none_kernel(uint32_t *__restrict__ idx, double *__restrict__ d2, size_t n) {
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) {
        idx[i] = ICP_NONE;
        d2[i] = INFINITY;
    }
}

template <bool SPARSE>
__global__ void __launch_bounds__(QB) icp_correspond_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted,
                                                           const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count,
                                                           const uint32_t *__restrict__ cell_count2, IcpArgs A) {
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    if (qi >= A.ns) return;
    const float sf[3] = {A.sx[qi], A.sy[qi], A.sz[qi]};
    double q[3];
    icp_move(A.T, sf[0], sf[1], sf[2], q);
    double best = INFINITY;
    uint32_t best_idx = ICP_NONE;
    const bool finite = isfinite(sf[0]) && isfinite(sf[1]) && isfinite(sf[2]) && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
    if (!finite) {
        A.idx[qi] = ICP_NONE;
        A.d2[qi] = INFINITY;
        return;
    }
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {   // floor((p - mn) * inv_h), clamped (before the conversion: the value may be beyond an int)
        double f = floor((q[a] - (double)g.mn[a]) * g.inv_h);
        f = f < 0.0 ? 0.0 : f;
        c[a] = f >= (double)g.dim[a] ? g.dim[a] - 1 : (int)f;
    }
    // what a candidate has to stay under (an equal one with a smaller index is taken too: see candidate)
    auto limit = [&]() { return fmin(best, A.max2); };
    auto candidate = [&](const float4 p) {
        const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const uint32_t id = __float_as_uint(p.w);
        if (d2 < A.max2 && (d2 < best || (d2 == best && id < best_idx))) {
            best = d2;
            best_idx = id;
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
    A.idx[qi] = best_idx;
    A.d2[qi] = best_idx == ICP_NONE ? INFINITY : best;
}

void launch_correspond(const GridView &v, const IcpArgs &A, hipStream_t s) {
    const unsigned qgrid = (unsigned)((A.ns + QB - 1) / QB);
    if (v.sparse)
        CW_LAUNCH("icp_correspond", (icp_correspond_kernel<true>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.starts, v.counts, v.counts2, A);
    else
        CW_LAUNCH("icp_correspond", (icp_correspond_kernel<false>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.starts, v.counts, v.counts2, A);
}

// ---- the sums ----
constexpr size_t ICP_CHUNK = 1024;        // source points per chunk before the shift (four per lane and step)
constexpr size_t ICP_MAX_CHUNKS = 1024;
constexpr int ICP_NSUM = 17;              // n, sum a, sum b, sum a b^T, sum d2
constexpr int ICP_FINAL_THREADS = 64;

struct IcpSumArgs {
    const float *sx, *sy, *sz;   // source planes (padded to a multiple of 256 points: a lane's four points are one 16-byte load)
    size_t ns;
    const uint32_t *idx;         // the search's results, arrays padded to a multiple of 4 entries
    const double *d2;
    const float *rx, *ry, *rz;   // the reference cloud's planes, in the original order idx refers to
    size_t nr;
    double T[12];
    double cp[3], cq[3];
    size_t chunk;
};

__global__ void __launch_bounds__(GRID_BLK) icp_sums_partial_kernel(IcpSumArgs A, double *__restrict__ partial /* [chunks][ICP_NSUM] */) {
    __shared__ double red[GRID_BLK / 64][ICP_NSUM];
    const size_t lo = (size_t)blockIdx.x * A.chunk, hi = lo + A.chunk < A.ns ? lo + A.chunk : A.ns;
    double s[ICP_NSUM];
#pragma unroll
    for (int v = 0; v < ICP_NSUM; v++) s[v] = 0.0;
    // (chunk is a multiple of 4 * GRID_BLK: a lane's points are the same whatever the launch looks like)
    for (size_t base = lo + 4 * (size_t)threadIdx.x; base < hi; base += 4 * (size_t)GRID_BLK) {
        const float4 x4 = *reinterpret_cast<const float4 *>(A.sx + base), y4 = *reinterpret_cast<const float4 *>(A.sy + base),
                     z4 = *reinterpret_cast<const float4 *>(A.sz + base);
        const uint4 i4 = *reinterpret_cast<const uint4 *>(A.idx + base);
        const double2 da = *reinterpret_cast<const double2 *>(A.d2 + base), db = *reinterpret_cast<const double2 *>(A.d2 + base + 2);
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
        const uint32_t is[4] = {i4.x, i4.y, i4.z, i4.w};
        const double ds[4] = {da.x, da.y, db.x, db.y};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            // (idx is checked against the reference count before it is an address; ICP_NONE fails the test too)
            if (base + u >= hi || (size_t)is[u] >= A.nr) continue;
            double p[3];
            icp_move(A.T, xs[u], ys[u], zs[u], p);
            const double a[3] = {p[0] - A.cp[0], p[1] - A.cp[1], p[2] - A.cp[2]};
            const double b[3] = {(double)A.rx[is[u]] - A.cq[0], (double)A.ry[is[u]] - A.cq[1], (double)A.rz[is[u]] - A.cq[2]};
            s[0] += 1.0;   // (a count below 2^53 is exact in f64)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                s[1 + i] += a[i];
                s[4 + i] += b[i];
#pragma unroll
                for (int j = 0; j < 3; j++) s[7 + 3 * i + j] += a[i] * b[j];
            }
            s[16] += ds[u];
        }
    }
#pragma unroll
    for (int v = 0; v < ICP_NSUM; v++) {
        for (int off = 32; off > 0; off >>= 1) s[v] += __shfl_down(s[v], off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][v] = s[v];
    }
    __syncthreads();
    if (threadIdx.x < ICP_NSUM) {
        double t = 0.0;
        for (int w = 0; w < GRID_BLK / 64; w++) t += red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * ICP_NSUM + threadIdx.x] = t;
    }
}

// out: 18 pinned 64-bit words -- n as an integer, the 16 sums, the tag
__global__ void __launch_bounds__(ICP_FINAL_THREADS) icp_sums_final_kernel(const double *__restrict__ partial, size_t nchunks, unsigned long long *__restrict__ out,
                                                                          unsigned long long tag) {
    const int v = threadIdx.x;
    if (v >= ICP_NSUM) return;
    double acc = 0.0;
    for (size_t c = 0; c < nchunks; c++) acc += partial[c * ICP_NSUM + v];
    if (v == 0) {
        out[0] = (unsigned long long)acc;
        out[ICP_NSUM] = tag;
    } else {
        out[v] = (unsigned long long)__double_as_longlong(acc);
    }
}

// ---- the sums of a plane fit (the contract is at the top of the file) ----
constexpr int ICP_PLANE_NSUM = 30;        // n, sum J J^T (21), sum J r (6), sum r^2, sum d2

struct IcpPlaneSumArgs {
    const float *sx, *sy, *sz;   // as IcpSumArgs
    size_t ns;
    const uint32_t *idx;
    const double *d2;
    const float *rx, *ry, *rz;   // the reference cloud's planes
    const float *mx, *my, *mz;   // its normals' planes, in the same order
    size_t nr;
    double T[12];
    size_t chunk;
};

__global__ void __launch_bounds__(GRID_BLK) icp_plane_sums_partial_kernel(IcpPlaneSumArgs A, double *__restrict__ partial /* [chunks][ICP_PLANE_NSUM] */) {
    __shared__ double red[GRID_BLK / 64][ICP_PLANE_NSUM];
    const size_t lo = (size_t)blockIdx.x * A.chunk, hi = lo + A.chunk < A.ns ? lo + A.chunk : A.ns;
    double s[ICP_PLANE_NSUM];
#pragma unroll
    for (int v = 0; v < ICP_PLANE_NSUM; v++) s[v] = 0.0;
    for (size_t base = lo + 4 * (size_t)threadIdx.x; base < hi; base += 4 * (size_t)GRID_BLK) {
        const float4 x4 = *reinterpret_cast<const float4 *>(A.sx + base), y4 = *reinterpret_cast<const float4 *>(A.sy + base),
                     z4 = *reinterpret_cast<const float4 *>(A.sz + base);
        const uint4 i4 = *reinterpret_cast<const uint4 *>(A.idx + base);
        const double2 da = *reinterpret_cast<const double2 *>(A.d2 + base), db = *reinterpret_cast<const double2 *>(A.d2 + base + 2);
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
        const uint32_t is[4] = {i4.x, i4.y, i4.z, i4.w};
        const double ds[4] = {da.x, da.y, db.x, db.y};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            // (idx is checked against the reference count before it is an address; ICP_NONE fails the test too)
            if (base + u >= hi || (size_t)is[u] >= A.nr) continue;
            double p[3];
            icp_move(A.T, xs[u], ys[u], zs[u], p);
            const double q[3] = {(double)A.rx[is[u]], (double)A.ry[is[u]], (double)A.rz[is[u]]};
            const double m[3] = {(double)A.mx[is[u]], (double)A.my[is[u]], (double)A.mz[is[u]]};
            const double e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
            const double r = (e[0] * m[0] + e[1] * m[1]) + e[2] * m[2];
            const double J[6] = {p[1] * m[2] - p[2] * m[1], p[2] * m[0] - p[0] * m[2], p[0] * m[1] - p[1] * m[0], m[0], m[1], m[2]};
            s[0] += 1.0;   // (a count below 2^53 is exact in f64)
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = i; j < 6; j++) s[1 + (i * (11 - i)) / 2 + j] += J[i] * J[j];   // (row i of the triangle begins at i (13 - i) / 2)
#pragma unroll
            for (int i = 0; i < 6; i++) s[22 + i] += J[i] * r;
            s[28] += r * r;
            s[29] += ds[u];
        }
    }
#pragma unroll
    for (int v = 0; v < ICP_PLANE_NSUM; v++) {
        for (int off = 32; off > 0; off >>= 1) s[v] += __shfl_down(s[v], off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][v] = s[v];
    }
    __syncthreads();
    if (threadIdx.x < ICP_PLANE_NSUM) {
        double t = 0.0;
        for (int w = 0; w < GRID_BLK / 64; w++) t += red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * ICP_PLANE_NSUM + threadIdx.x] = t;
    }
}

// out: 31 pinned 64-bit words -- n as an integer, the 29 sums, the tag
__global__ void __launch_bounds__(ICP_FINAL_THREADS) icp_plane_sums_final_kernel(const double *__restrict__ partial, size_t nchunks,
                                                                                unsigned long long *__restrict__ out, unsigned long long tag) {
    const int v = threadIdx.x;
    if (v >= ICP_PLANE_NSUM) return;
    double acc = 0.0;
    for (size_t c = 0; c < nchunks; c++) acc += partial[c * ICP_PLANE_NSUM + v];
    if (v == 0) {
        out[0] = (unsigned long long)acc;
        out[ICP_PLANE_NSUM] = tag;
    } else {
        out[v] = (unsigned long long)__double_as_longlong(acc);
    }
}

// Device memory of one search: d2 | idx | partial sums, one pool block.
struct IcpWork {
    char *block = nullptr;
    uint32_t *idx = nullptr;
    double *d2 = nullptr;
    double *partial = nullptr;
    size_t chunk = 0, nchunks = 0;
    bool alloc(size_t ns, int nsum = ICP_NSUM) {   // nsum: values per chunk in `partial`
        chunk = ICP_CHUNK;
        while ((ns + chunk - 1) / chunk > ICP_MAX_CHUNKS) chunk <<= 1;
        nchunks = (ns + chunk - 1) / chunk;
        const size_t padded = (ns + 255) & ~(size_t)255;
        const size_t idx_bytes = padded * sizeof(uint32_t), d2_bytes = padded * sizeof(double);
        block = (char *)pool_alloc(idx_bytes + d2_bytes + nchunks * (size_t)nsum * sizeof(double));
        if (!block) return false;
        d2 = (double *)block;   // (both arrays start on a 1 KiB boundary of the block: 16-byte loads)
        idx = (uint32_t *)(block + d2_bytes);
        partial = (double *)(block + d2_bytes + idx_bytes);
        return true;
    }
    ~IcpWork() { pool_free(block); }   // (the owner has waited for the stream)
};

IcpArgs correspond_args(const DeviceSoA &source, const double T[16], double max_distance, const IcpWork &w) {
    IcpArgs A{};
    A.sx = source.x(); A.sy = source.y(); A.sz = source.z();
    A.ns = source.npoints;
    for (int i = 0; i < 12; i++) A.T[i] = T[i];
    A.max2 = max_distance * max_distance;
    A.idx = w.idx;
    A.d2 = w.d2;
    return A;
}

// the two sums kernels behind a search on stream s; the result lands in the thread's pinned words under `tag`
void launch_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], const double cp[3], const double cq[3], const IcpWork &w,
                 ThreadCtx &c, uint32_t tag, hipStream_t s) {
    IcpSumArgs S{};
    S.sx = source.x(); S.sy = source.y(); S.sz = source.z();
    S.ns = source.npoints;
    S.idx = w.idx;
    S.d2 = w.d2;
    S.rx = reference.x(); S.ry = reference.y(); S.rz = reference.z();
    S.nr = reference.npoints;
    for (int i = 0; i < 12; i++) S.T[i] = T[i];
    for (int a = 0; a < 3; a++) { S.cp[a] = cp[a]; S.cq[a] = cq[a]; }
    S.chunk = w.chunk;
    CW_LAUNCH("icp_sums_partial", icp_sums_partial_kernel, dim3((unsigned)w.nchunks), dim3(GRID_BLK), 0, s, S, w.partial);
    CW_LAUNCH("icp_sums_final", icp_sums_final_kernel, dim3(1), dim3(ICP_FINAL_THREADS), 0, s, w.partial, w.nchunks,
              reinterpret_cast<unsigned long long *>(c.host_words), (unsigned long long)tag);
}

// after a wait on the stream: the pinned words into n and sums
bool read_sums(ThreadCtx &c, uint32_t tag, uint64_t *n, double sums[16]) {
    const volatile unsigned long long *words = reinterpret_cast<const volatile unsigned long long *>(c.host_words);
    if (words[ICP_NSUM] != (unsigned long long)tag) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_icp", "the sums kernel did not report");
        return false;
    }
    *n = words[0];
    for (int v = 0; v < 16; v++) {
        const unsigned long long bits = words[1 + v];
        memcpy(&sums[v], &bits, sizeof(double));
    }
    return true;
}

uint32_t next_tag(ThreadCtx &c) {
    volatile unsigned long long *words = reinterpret_cast<volatile unsigned long long *>(c.host_words);
    words[ICP_NSUM] = 0ull;
    return ++c.tag ? c.tag : ++c.tag;
}

bool icp_args_ok(const char *who, const double T[16], double max_distance) {
    if (!(max_distance > 0.0)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_distance must be positive (inf: no bound)");
        return false;
    }
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(T[i])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the matrix must be finite");
            return false;
        }
    return true;
}

}  // namespace

bool icp_correspondences(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, uint32_t *idx_host,
                         double *d2_host) {
    const char *who = "cwipc_hip_correspondences";
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (!icp_args_ok(who, T, max_distance)) return false;
    const size_t ns = source.npoints;
    if (ns == 0) return true;
    IcpWork w;
    if (!w.alloc(ns)) return false;
    bool ok;
    if (reference.npoints == 0) {
        CW_LAUNCH("icp_fill_none", icp_fill_none_kernel, dim3(grid_blocks(ns)), dim3(GRID_BLK), 0, c.stream, w.idx, w.d2, ns);
        ok = hipGetLastError() == hipSuccess;
    } else {
        const IcpArgs A = correspond_args(source, T, max_distance, w);
        const GridSearch search = [&](const GridView &v, hipStream_t s) {
            launch_correspond(v, A, s);
            return hipGetLastError() == hipSuccess;
        };
        ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    }
    if (idx_host) ok = ok && hipMemcpyAsync(idx_host, w.idx, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    if (d2_host) ok = ok && hipMemcpyAsync(d2_host, w.d2, ns * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;   // (also on failure: kernels that write the block may still be in flight)
    return ok;
}

bool icp_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, const double cp[3], const double cq[3],
              uint64_t *n, double sums[16]) {
    const char *who = "cwipc_hip_icp_sums";
    *n = 0;
    for (int v = 0; v < 16; v++) sums[v] = 0.0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (!icp_args_ok(who, T, max_distance)) return false;
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(cp[a]) || !std::isfinite(cq[a])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the pivots must be finite");
            return false;
        }
    const size_t ns = source.npoints;
    if (ns == 0 || reference.npoints == 0) return true;
    IcpWork w;
    if (!w.alloc(ns)) return false;
    const IcpArgs A = correspond_args(source, T, max_distance, w);
    const uint32_t tag = next_tag(c);
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        launch_correspond(v, A, s);
        launch_sums(source, reference, T, cp, cq, w, c, tag, s);
        return hipGetLastError() == hipSuccess;
    };
    bool ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    ok = c.sync() && ok;
    return ok && read_sums(c, tag, n, sums);
}

bool icp_point2point(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const double init[16], double relative_fitness,
                     double relative_rmse, int max_iteration, const double cp0[3], const double cq[3], double T_out[16], double *fitness,
                     double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_point2point";
    for (int i = 0; i < 16; i++) T_out[i] = init[i];
    *fitness = 0.0;
    *inlier_rmse = 0.0;
    *iterations = 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (!icp_args_ok(who, init, max_distance)) return false;
    if (max_iteration < 0 || std::isnan(relative_fitness) || std::isnan(relative_rmse)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_iteration must not be negative, the criteria not NaN");
        return false;
    }
    const size_t ns = source.npoints;
    if (ns == 0 || reference.npoints == 0) return true;
    IcpWork w;
    if (!w.alloc(ns)) return false;
    bool loop_ok = true;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        double T[16];
        for (int i = 0; i < 16; i++) T[i] = init[i];
        // one evaluation: search, sums, wait, read
        uint64_t n = 0;
        double sums[16], cp[3];
        auto evaluate = [&]() {
            // cp = T applied to the source's centroid: the pivot follows the cloud
            for (int r = 0; r < 3; r++) cp[r] = ((T[4 * r] * cp0[0] + T[4 * r + 1] * cp0[1]) + T[4 * r + 2] * cp0[2]) + T[4 * r + 3];
            const IcpArgs A = correspond_args(source, T, max_distance, w);
            const uint32_t tag = next_tag(c);
            launch_correspond(v, A, s);
            launch_sums(source, reference, T, cp, cq, w, c, tag, s);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
            return read_sums(c, tag, &n, sums);
        };
        auto measures = [&](double &fit, double &rmse) {
            fit = n ? (double)n / (double)ns : 0.0;
            rmse = n ? sqrt(sums[15] / (double)n) : 0.0;
        };
        if (!evaluate()) return loop_ok = false;
        double fit, rmse;
        measures(fit, rmse);
        int done = 0;
        if (n != 0) {
            for (int it = 0; it < max_iteration; it++) {
                double R[3][3], t[3];
                rigid_fit(n, sums, sums + 3, sums + 6, cp, cq, R, t);
                double U[16] = {R[0][0], R[0][1], R[0][2], t[0], R[1][0], R[1][1], R[1][2], t[1], R[2][0], R[2][1], R[2][2], t[2], 0, 0, 0, 1}, N[16];
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++) N[4 * i + j] = ((U[4 * i] * T[j] + U[4 * i + 1] * T[4 + j]) + U[4 * i + 2] * T[8 + j]) + U[4 * i + 3] * T[12 + j];
                for (int i = 0; i < 16; i++) T[i] = N[i];
                for (int i = 0; i < 16; i++)
                    if (!std::isfinite(T[i])) {
                        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the transformation is no longer finite");
                        return loop_ok = false;
                    }
                const double fit_before = fit, rmse_before = rmse;
                if (!evaluate()) return loop_ok = false;
                measures(fit, rmse);
                done = it + 1;
                if (fabs(fit_before - fit) < relative_fitness && fabs(rmse_before - rmse) < relative_rmse) break;
            }
        }
        for (int i = 0; i < 16; i++) T_out[i] = T[i];
        *fitness = fit;
        *inlier_rmse = rmse;
        *iterations = done;
        return true;
    };
    bool ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    ok = c.sync() && ok;
    return ok && loop_ok;
}

// ---- point-to-plane: the host side ----
namespace {

void launch_plane_sums(const DeviceSoA &source, const DeviceSoA &reference, const float *normals, const double T[16], const IcpWork &w, ThreadCtx &c,
                       uint32_t tag, hipStream_t s) {
    IcpPlaneSumArgs S{};
    S.sx = source.x(); S.sy = source.y(); S.sz = source.z();
    S.ns = source.npoints;
    S.idx = w.idx;
    S.d2 = w.d2;
    S.rx = reference.x(); S.ry = reference.y(); S.rz = reference.z();
    S.nr = reference.npoints;
    S.mx = normals; S.my = normals + S.nr; S.mz = normals + 2 * S.nr;
    for (int i = 0; i < 12; i++) S.T[i] = T[i];
    S.chunk = w.chunk;
    CW_LAUNCH("icp_plane_sums_partial", icp_plane_sums_partial_kernel, dim3((unsigned)w.nchunks), dim3(GRID_BLK), 0, s, S, w.partial);
    CW_LAUNCH("icp_plane_sums_final", icp_plane_sums_final_kernel, dim3(1), dim3(ICP_FINAL_THREADS), 0, s, w.partial, w.nchunks,
              reinterpret_cast<unsigned long long *>(c.host_words), (unsigned long long)tag);
}

bool read_plane_sums(ThreadCtx &c, uint32_t tag, uint64_t *n, double sums[29]) {
    const volatile unsigned long long *words = reinterpret_cast<const volatile unsigned long long *>(c.host_words);
    if (words[ICP_PLANE_NSUM] != (unsigned long long)tag) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_icp", "the plane sums kernel did not report");
        return false;
    }
    *n = words[0];
    for (int v = 0; v < ICP_PLANE_NSUM - 1; v++) {
        const unsigned long long bits = words[1 + v];
        memcpy(&sums[v], &bits, sizeof(double));
    }
    return true;
}

uint32_t next_plane_tag(ThreadCtx &c) {
    volatile unsigned long long *words = reinterpret_cast<volatile unsigned long long *>(c.host_words);
    words[ICP_PLANE_NSUM] = 0ull;
    return ++c.tag ? c.tag : ++c.tag;
}

// The reference cloud's normals as three planes of count(reference) floats in one pool block (and, behind them, the three doubles
// direction_normals wants for its centroid): the caller's, copied, or estimated there.  On the calling thread's stream, no wait.
struct IcpNormals {
    float *planes = nullptr;
    bool make(const char *who, const DeviceSoA &reference, const float *host_normals, float radius, int max_nn, ThreadCtx &c) {
        const size_t nr = reference.npoints;
        const size_t cen_at = (3 * nr * sizeof(float) + 127) & ~(size_t)127;
        planes = (float *)pool_alloc(cen_at + 3 * sizeof(double));
        if (!planes) return false;
        if (host_normals) {
            for (size_t i = 0; i < 3 * nr; i++)
                if (!std::isfinite(host_normals[i])) {
                    cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the normals must be finite");
                    return false;
                }
            return hipMemcpyAsync(planes, host_normals, 3 * nr * sizeof(float), hipMemcpyHostToDevice, c.stream) == hipSuccess;
        }
        const double zero[3] = {0, 0, 0};
        double *cen = reinterpret_cast<double *>(reinterpret_cast<char *>(planes) + cen_at);
        return direction_normals(reference, radius, max_nn, zero, 0.0, nullptr, planes, nr, nullptr, cen);
    }
    ~IcpNormals() { pool_free(planes); }   // (the owner has waited for the stream)
};

bool plane_args_ok(const char *who, const float *host_normals, float radius, int max_nn) {
    if (host_normals || (radius > 0.f && std::isfinite(radius) && max_nn >= 1 && max_nn <= DIRECTION_MAX_NN)) return true;
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "radius must be positive and finite, max_nn between 1 and 128");
    return false;
}

// The loop of the aligners whose update is plane_fit's (point-to-plane and generalized ICP): they differ in the sums kernel that
// follows the search, which `launch` puts on the stream; the sums have one layout.  Inside ONE grid hook; waits for its results.
using PlaneSumsLaunch = std::function<void(const double T[16], uint32_t tag, hipStream_t s)>;

bool plane_loop(const char *who, const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const double init[16], double relative_fitness,
                double relative_rmse, int max_iteration, const IcpWork &w, ThreadCtx &c, const PlaneSumsLaunch &launch, double T_out[16],
                double *fitness, double *inlier_rmse, int *iterations) {
    const size_t ns = source.npoints;
    bool loop_ok = true;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        double T[16];
        for (int i = 0; i < 16; i++) T[i] = init[i];
        // one evaluation: search, sums, wait, read
        uint64_t n = 0;
        double sums[29];
        auto evaluate = [&]() {
            const IcpArgs A = correspond_args(source, T, max_distance, w);
            const uint32_t tag = next_plane_tag(c);
            launch_correspond(v, A, s);
            launch(T, tag, s);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
            return read_plane_sums(c, tag, &n, sums);
        };
        auto measures = [&](double &fit, double &rmse) {
            fit = n ? (double)n / (double)ns : 0.0;
            rmse = n ? sqrt(sums[28] / (double)n) : 0.0;
        };
        if (!evaluate()) return loop_ok = false;
        double fit, rmse;
        measures(fit, rmse);
        int done = 0;
        if (n != 0) {
            for (int it = 0; it < max_iteration; it++) {
                double R[3][3], t[3];
                plane_fit(sums, sums + 21, R, t);
                double U[16] = {R[0][0], R[0][1], R[0][2], t[0], R[1][0], R[1][1], R[1][2], t[1], R[2][0], R[2][1], R[2][2], t[2], 0, 0, 0, 1}, N[16];
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++) N[4 * i + j] = ((U[4 * i] * T[j] + U[4 * i + 1] * T[4 + j]) + U[4 * i + 2] * T[8 + j]) + U[4 * i + 3] * T[12 + j];
                for (int i = 0; i < 16; i++) T[i] = N[i];
                for (int i = 0; i < 16; i++)
                    if (!std::isfinite(T[i])) {
                        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the transformation is no longer finite");
                        return loop_ok = false;
                    }
                const double fit_before = fit, rmse_before = rmse;
                if (!evaluate()) return loop_ok = false;
                measures(fit, rmse);
                done = it + 1;
                if (fabs(fit_before - fit) < relative_fitness && fabs(rmse_before - rmse) < relative_rmse) break;
            }
        }
        for (int i = 0; i < 16; i++) T_out[i] = T[i];
        *fitness = fit;
        *inlier_rmse = rmse;
        *iterations = done;
        return true;
    };
    bool ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    ok = c.sync() && ok;
    return ok && loop_ok;
}

}  // namespace

bool icp_plane_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, const float *host_normals, float radius,
                    int max_nn, uint64_t *n, double sums[29]) {
    const char *who = "cwipc_hip_icp_plane_sums";
    *n = 0;
    for (int v = 0; v < 29; v++) sums[v] = 0.0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (!icp_args_ok(who, T, max_distance) || !plane_args_ok(who, host_normals, radius, max_nn)) return false;
    const size_t ns = source.npoints;
    if (reference.npoints == 0) return true;
    IcpNormals normals;
    IcpWork w;
    // (the caller's normals are looked at even when there is nothing to match them with: a bad array is an error either way)
    bool ok = normals.make(who, reference, host_normals, radius, max_nn, c);
    if (ok && ns != 0) ok = w.alloc(ns, ICP_PLANE_NSUM);
    if (!ok || ns == 0) return c.sync() && ok;   // (a wait also on failure: kernels that write the blocks may still be in flight)
    const IcpArgs A = correspond_args(source, T, max_distance, w);
    const uint32_t tag = next_plane_tag(c);
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        launch_correspond(v, A, s);
        launch_plane_sums(source, reference, normals.planes, T, w, c, tag, s);
        return hipGetLastError() == hipSuccess;
    };
    ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    ok = c.sync() && ok;
    return ok && read_plane_sums(c, tag, n, sums);
}

bool icp_point2plane(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const double init[16], const float *host_normals,
                     float radius, int max_nn, double relative_fitness, double relative_rmse, int max_iteration, double T_out[16], double *fitness,
                     double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_point2plane";
    for (int i = 0; i < 16; i++) T_out[i] = init[i];
    *fitness = 0.0;
    *inlier_rmse = 0.0;
    *iterations = 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (!icp_args_ok(who, init, max_distance) || !plane_args_ok(who, host_normals, radius, max_nn)) return false;
    if (max_iteration < 0 || std::isnan(relative_fitness) || std::isnan(relative_rmse)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_iteration must not be negative, the criteria not NaN");
        return false;
    }
    const size_t ns = source.npoints;
    if (reference.npoints == 0) return true;
    IcpNormals normals;
    IcpWork w;
    // the normals, once per run and before the grid hook: direction_normals builds a grid of its own width
    bool ok = normals.make(who, reference, host_normals, radius, max_nn, c);
    if (ok && ns != 0) ok = w.alloc(ns, ICP_PLANE_NSUM);
    if (!ok || ns == 0) return c.sync() && ok;
    const PlaneSumsLaunch launch = [&](const double T[16], uint32_t tag, hipStream_t s) {
        launch_plane_sums(source, reference, normals.planes, T, w, c, tag, s);
    };
    return plane_loop(who, source, reference, max_distance, init, relative_fitness, relative_rmse, max_iteration, w, c, launch, T_out, fitness,
                      inlier_rmse, iterations);
}

// ---- generalized ICP (the contract is stated in include/cwipc_util_amd/hip_ext.h; the arithmetic is gicp_terms.hpp) ----
namespace {

// Per point of a cloud the covariance of gicp_terms.hpp from its normal: value v of point i goes to cov[i * point_stride + v *
// value_stride], which writes either layout the sums kernel reads -- six planes for the source (point_stride 1, value_stride the
// padded count: a lane's four points are two 16-byte loads per plane, in order) and records of six doubles for the reference
// (point_stride 6, value_stride 1: a gathered record is 48 bytes, three 16-byte loads in at most two cache lines).
struct GicpCovArgs {
    const float *mx, *my, *mz;   // the normals' planes
    size_t n;
    double dir[3];               // the cloud's direction
    int orient;                  // 0: the normals are taken as they are
    double eps;
    double *cov;
    size_t point_stride, value_stride;
};

__global__ void __launch_bounds__(GRID_BLK) gicp_covariance_kernel(GicpCovArgs A) {
    const size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x;
    if (i >= A.n) return;
    double m[3] = {(double)A.mx[i], (double)A.my[i], (double)A.mz[i]};
    if (A.orient) gicp_orient(m, A.dir);
    double C[6];
    gicp_covariance(m, A.eps, C);
#pragma unroll
    for (int v = 0; v < 6; v++) A.cov[i * A.point_stride + (size_t)v * A.value_stride] = C[v];
}

struct IcpGicpSumArgs {
    const float *sx, *sy, *sz;   // as IcpSumArgs
    size_t ns;
    const uint32_t *idx;
    const double *d2;
    const float *rx, *ry, *rz;   // the reference cloud's planes
    size_t nr;
    const double *cs;            // the source's covariances: six planes of cs_stride doubles (cs_stride a multiple of 256)
    size_t cs_stride;
    const double *ct;            // the reference's: nr records of six doubles
    double T[12];
    size_t chunk;
};

// The shape of icp_plane_sums_partial_kernel: the same chunks, four points per lane and step in index order, the same trees.
__global__ void __launch_bounds__(GRID_BLK) icp_gicp_sums_partial_kernel(IcpGicpSumArgs A, double *__restrict__ partial /* [chunks][GICP_NTERM] */) {
    __shared__ double red[GRID_BLK / 64][GICP_NTERM];
    const size_t lo = (size_t)blockIdx.x * A.chunk, hi = lo + A.chunk < A.ns ? lo + A.chunk : A.ns;
    const double R[9] = {A.T[0], A.T[1], A.T[2], A.T[4], A.T[5], A.T[6], A.T[8], A.T[9], A.T[10]};
    double s[GICP_NTERM];
#pragma unroll
    for (int v = 0; v < GICP_NTERM; v++) s[v] = 0.0;
    for (size_t base = lo + 4 * (size_t)threadIdx.x; base < hi; base += 4 * (size_t)GRID_BLK) {
        const float4 x4 = *reinterpret_cast<const float4 *>(A.sx + base), y4 = *reinterpret_cast<const float4 *>(A.sy + base),
                     z4 = *reinterpret_cast<const float4 *>(A.sz + base);
        const uint4 i4 = *reinterpret_cast<const uint4 *>(A.idx + base);
        const double2 da = *reinterpret_cast<const double2 *>(A.d2 + base), db = *reinterpret_cast<const double2 *>(A.d2 + base + 2);
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
        const uint32_t is[4] = {i4.x, i4.y, i4.z, i4.w};
        const double ds[4] = {da.x, da.y, db.x, db.y};
        double cs[4][6];
#pragma unroll
        for (int v = 0; v < 6; v++) {
            const double2 ca = *reinterpret_cast<const double2 *>(A.cs + (size_t)v * A.cs_stride + base),
                          cb = *reinterpret_cast<const double2 *>(A.cs + (size_t)v * A.cs_stride + base + 2);
            cs[0][v] = ca.x; cs[1][v] = ca.y; cs[2][v] = cb.x; cs[3][v] = cb.y;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            // (idx is checked against the reference count before it is an address; ICP_NONE fails the test too)
            if (base + u >= hi || (size_t)is[u] >= A.nr) continue;
            double p[3];
            icp_move(A.T, xs[u], ys[u], zs[u], p);
            const double q[3] = {(double)A.rx[is[u]], (double)A.ry[is[u]], (double)A.rz[is[u]]};
            const double2 *rec = reinterpret_cast<const double2 *>(A.ct + 6 * (size_t)is[u]);
            const double2 c0 = rec[0], c1 = rec[1], c2 = rec[2];
            const double ct[6] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y};
            double t[GICP_NTERM];
            gicp_pair_terms(p, q, cs[u], ct, R, ds[u], t);
#pragma unroll
            for (int v = 0; v < GICP_NTERM; v++) s[v] += t[v];   // (t[0] is 1: a count below 2^53 is exact in f64)
        }
    }
#pragma unroll
    for (int v = 0; v < GICP_NTERM; v++) {
        for (int off = 32; off > 0; off >>= 1) s[v] += __shfl_down(s[v], off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][v] = s[v];
    }
    __syncthreads();
    if (threadIdx.x < GICP_NTERM) {
        double t = 0.0;
        for (int w = 0; w < GRID_BLK / 64; w++) t += red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * GICP_NTERM + threadIdx.x] = t;
    }
}
static_assert(GICP_NTERM == ICP_PLANE_NSUM, "the generalized sums go through the plane sums' final kernel and pinned words");

// A cloud's covariances in one pool block, in either layout of gicp_covariance_kernel.  On the calling thread's stream, no wait.
struct GicpCov {
    double *values = nullptr;
    size_t stride = 0;   // planes: the padded count
    bool make(const DeviceSoA &cloud, const float *normal_planes, const double *direction, double eps, bool records, ThreadCtx &c) {
        const size_t n = cloud.npoints;
        stride = (n + 255) & ~(size_t)255;
        values = (double *)pool_alloc(6 * (records ? n : stride) * sizeof(double));
        if (!values) return false;
        GicpCovArgs A{};
        A.mx = normal_planes; A.my = normal_planes + n; A.mz = normal_planes + 2 * n;
        A.n = n;
        A.orient = direction != nullptr;
        for (int a = 0; a < 3; a++) A.dir[a] = direction ? direction[a] : 0.0;
        A.eps = eps;
        A.cov = values;
        A.point_stride = records ? 6 : 1;
        A.value_stride = records ? 1 : stride;
        CW_LAUNCH("gicp_covariance", gicp_covariance_kernel, dim3((unsigned)((n + GRID_BLK - 1) / GRID_BLK)), dim3(GRID_BLK), 0, c.stream, A);
        return hipGetLastError() == hipSuccess;
    }
    ~GicpCov() { pool_free(values); }   // (the owner has waited for the stream)
};

void launch_gicp_sums(const DeviceSoA &source, const DeviceSoA &reference, const GicpCov &cs, const GicpCov &ct, const double T[16], const IcpWork &w,
                      ThreadCtx &c, uint32_t tag, hipStream_t s) {
    IcpGicpSumArgs S{};
    S.sx = source.x(); S.sy = source.y(); S.sz = source.z();
    S.ns = source.npoints;
    S.idx = w.idx;
    S.d2 = w.d2;
    S.rx = reference.x(); S.ry = reference.y(); S.rz = reference.z();
    S.nr = reference.npoints;
    S.cs = cs.values;
    S.cs_stride = cs.stride;
    S.ct = ct.values;
    for (int i = 0; i < 12; i++) S.T[i] = T[i];
    S.chunk = w.chunk;
    CW_LAUNCH("icp_gicp_sums_partial", icp_gicp_sums_partial_kernel, dim3((unsigned)w.nchunks), dim3(GRID_BLK), 0, s, S, w.partial);
    CW_LAUNCH("icp_plane_sums_final", icp_plane_sums_final_kernel, dim3(1), dim3(ICP_FINAL_THREADS), 0, s, w.partial, w.nchunks,
              reinterpret_cast<unsigned long long *>(c.host_words), (unsigned long long)tag);
}

bool gicp_args_ok(const char *who, const float *source_normals, const float *reference_normals, float radius, int max_nn, double epsilon) {
    if (!(epsilon > 0.0) || !std::isfinite(epsilon)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "epsilon must be positive and finite");
        return false;
    }
    // (radius and max_nn matter when either cloud's normals are to be estimated)
    return plane_args_ok(who, source_normals && reference_normals ? source_normals : nullptr, radius, max_nn);
}

bool normals_finite(const char *who, const float *host_normals, size_t n) {
    for (size_t i = 0; host_normals && i < 3 * n; i++)
        if (!std::isfinite(host_normals[i])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the normals must be finite");
            return false;
        }
    return true;
}

// What both clouds need before the first search, once per run and before the grid hook: the two directions (the reference's
// _fix_normal_direction: from the midpoint of the two centroids towards each cloud's own), the normals, the covariances.
struct GicpClouds {
    IcpNormals source_normals, reference_normals;
    GicpCov cs, ct;
    bool make(const char *who, const DeviceSoA &source, const DeviceSoA &reference, const float *host_source_normals, const float *host_reference_normals,
              float radius, int max_nn, double epsilon, ThreadCtx &c) {
        double cen_s[3], cen_t[3], ds[3], dt[3];
        if (!icp_centroid(source, cen_s) || !icp_centroid(reference, cen_t)) return false;
        for (int a = 0; a < 3; a++) {
            const double o = (cen_s[a] + cen_t[a]) / 2;
            ds[a] = cen_s[a] - o;
            dt[a] = cen_t[a] - o;
        }
        // (the source's normals are those of the original source cloud: T never reaches them, its rotation reaches the covariances)
        return source_normals.make(who, source, host_source_normals, radius, max_nn, c) &&
               reference_normals.make(who, reference, host_reference_normals, radius, max_nn, c) &&
               cs.make(source, source_normals.planes, ds, epsilon, false, c) && ct.make(reference, reference_normals.planes, dt, epsilon, true, c);
    }
};

}  // namespace

bool icp_gicp_covariances(const DeviceSoA &cloud, const float *host_normals, float radius, int max_nn, const double *direction, double epsilon,
                          double *cov_host) {
    const char *who = "cwipc_hip_gicp_covariances";
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (!gicp_args_ok(who, host_normals, host_normals, radius, max_nn, epsilon)) return false;
    const size_t n = cloud.npoints;
    if (n == 0) return true;
    IcpNormals normals;
    GicpCov cov;
    bool ok = normals.make(who, cloud, host_normals, radius, max_nn, c) && cov.make(cloud, normals.planes, direction, epsilon, true, c);
    ok = ok && hipMemcpyAsync(cov_host, cov.values, 6 * n * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    return c.sync() && ok;   // (a wait also on failure: kernels that write the blocks may still be in flight)
}

bool icp_gicp_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, const float *source_normals,
                   const float *reference_normals, float radius, int max_nn, double epsilon, uint64_t *n, double sums[29]) {
    const char *who = "cwipc_hip_icp_gicp_sums";
    *n = 0;
    for (int v = 0; v < 29; v++) sums[v] = 0.0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (!icp_args_ok(who, T, max_distance) || !gicp_args_ok(who, source_normals, reference_normals, radius, max_nn, epsilon)) return false;
    const size_t ns = source.npoints;
    // (the caller's normals are looked at even when there is nothing to match them with: a bad array is an error either way)
    if (!normals_finite(who, source_normals, ns) || !normals_finite(who, reference_normals, reference.npoints)) return false;
    if (ns == 0 || reference.npoints == 0) return true;
    GicpClouds clouds;
    IcpWork w;
    bool ok = clouds.make(who, source, reference, source_normals, reference_normals, radius, max_nn, epsilon, c) && w.alloc(ns, GICP_NTERM);
    if (!ok) return c.sync() && ok;   // (a wait also on failure: kernels that write the blocks may still be in flight)
    const IcpArgs A = correspond_args(source, T, max_distance, w);
    const uint32_t tag = next_plane_tag(c);
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        launch_correspond(v, A, s);
        launch_gicp_sums(source, reference, clouds.cs, clouds.ct, T, w, c, tag, s);
        return hipGetLastError() == hipSuccess;
    };
    ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    ok = c.sync() && ok;
    return ok && read_plane_sums(c, tag, n, sums);
}

bool icp_generalized(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const double init[16], const float *source_normals,
                     const float *reference_normals, float radius, int max_nn, double epsilon, double relative_fitness, double relative_rmse,
                     int max_iteration, double T_out[16], double *fitness, double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_generalized";
    for (int i = 0; i < 16; i++) T_out[i] = init[i];
    *fitness = 0.0;
    *inlier_rmse = 0.0;
    *iterations = 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (!icp_args_ok(who, init, max_distance) || !gicp_args_ok(who, source_normals, reference_normals, radius, max_nn, epsilon)) return false;
    if (max_iteration < 0 || std::isnan(relative_fitness) || std::isnan(relative_rmse)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_iteration must not be negative, the criteria not NaN");
        return false;
    }
    const size_t ns = source.npoints;
    if (!normals_finite(who, source_normals, ns) || !normals_finite(who, reference_normals, reference.npoints)) return false;
    if (ns == 0 || reference.npoints == 0) return true;
    GicpClouds clouds;
    IcpWork w;
    const bool ok = clouds.make(who, source, reference, source_normals, reference_normals, radius, max_nn, epsilon, c) && w.alloc(ns, GICP_NTERM);
    if (!ok) return c.sync() && ok;
    const PlaneSumsLaunch launch = [&](const double T[16], uint32_t tag, hipStream_t s) {
        launch_gicp_sums(source, reference, clouds.cs, clouds.ct, T, w, c, tag, s);
    };
    return plane_loop(who, source, reference, max_distance, init, relative_fitness, relative_rmse, max_iteration, w, c, launch, T_out, fitness,
                      inlier_rmse, iterations);
}

// the mean of the cloud's points (the direction filter's centroid kernels), on the host; non-finite where a point is
bool icp_centroid(const DeviceSoA &cloud, double cen[3]) {
    cen[0] = cen[1] = cen[2] = 0.0;
    if (cloud.npoints == 0) return true;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    double *dev = (double *)pool_alloc(3 * sizeof(double));
    double *host = (double *)c.staging(3 * sizeof(double));
    if (!dev || !host) { pool_free(dev); return false; }
    const double zero[3] = {0, 0, 0};
    bool ok = direction_normals(cloud, 1.f, 1, zero, 0.0, nullptr, nullptr, 0, nullptr, dev);
    ok = ok && hipMemcpyAsync(host, dev, 3 * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(dev);
    if (ok) for (int a = 0; a < 3; a++) cen[a] = host[a];
    return ok;
}

}  // namespace cwipc_amd
