// kernels_icp.hip -- ICP fine alignment on gfx950: point-to-point, point-to-plane and generalized (registration/fine.py and the
// overlap analyzer of registration/analyze.py).
//
// Reference: python/cwipc/registration/fine.py and analyze.py (OverlapAnalyzer), which call open3d's registration_icp /
// registration_generalized_icp and evaluate_registration on the CPU.  open3d is not on this stack: point-to-point is pinned by
// tests/icp_model.py, point-to-plane by tests/icp_plane_model.py, generalized ICP by tests/icp_gicp_model.py -- restatements of the
// published algorithms in numpy.  The three aligners are ONE search, ONE sums skeleton and ONE loop; an aligner is what a matched
// pair contributes to the sums (a `Pair` below) and how the sums become a motion (an update, on the host).
//
// 1. CORRESPONDENCES (icp_correspond_kernel), the same for every aligner.  One lane per SOURCE point, in the caller's order.  The
// query is the source point moved by the 4x4 matrix T (row-major f64), computed in f64 from the float32 coordinates (icp_move):
//     px = ((T00*x + T01*y) + T02*z) + T03        (py, pz alike; every operation rounded on its own, -ffp-contract=off)
// and searched in the point grid over the REFERENCE cloud by the exact walk of exact_walk.hpp (walk_exact: what nn_distance2_kernel
// of kernels_nn.hip walks, by construction), from the cell floor((p - mn) * inv_h) of the f64 value, clamped.  Per source point:
// idx = the ORIGINAL index (sorted[].w) of the nearest reference point, d2 = (dx*dx + dy*dy) + dz*dz with dx = px - (double)qx;
// only candidates with d2 < max_distance^2 (strictly) count; 0xFFFFFFFF and +inf when there is none, also for a source point with
// a non-finite coordinate before or after T.  Reference points with a non-finite coordinate are not in the grid and are never
// candidates.
//   AMONG EQUAL d2 THE SMALLEST ORIGINAL INDEX WINS.  The candidate test of the kernel says so for the candidates it is shown;
//   that it is shown every equally distant one, in whatever cell, is walk_exact's property (its bounds are short: see there).
//
// 2. SUMS (icp_sums_partial_kernel<Pair>, icp_sums_final_kernel<NSUM>).  Over the source points that have a correspondence, with p
// the moved source point (recomputed by icp_move, not stored) and q the matched reference point ((double) of float32), a Pair
// gives NSUM - 1 terms and the skeleton adds them up, with the count n in front.  The summation scheme is the contract that makes
// two calls give the same bytes, and it is stated here once: the source is cut into chunks of ICP_CHUNK << s points, s the
// smallest shift that leaves at most ICP_MAX_CHUNKS chunks -- a function of the source count alone; one workgroup per chunk; a
// lane takes four consecutive points per step (16-byte loads) and adds every term of a point to its accumulator in index order; a
// fixed shuffle tree closes the wave and the first NSUM lanes add the four waves in order; a second kernel adds the chunks in
// index order and writes n (as an integer), the NSUM - 1 sums and the tag, NSUM + 1 of the 32 pinned 64-bit words a thread has.
// No atomics.  idx is checked against the reference count before it is an address.  The Pairs, every operation rounded on its own:
//   PointPair (17): with pivots cp, cq (kernel arguments), a = p - cp and b = q - cq:
//       n | sum a (3) | sum b (3) | sum a b^T (9, row-major: a_i b_j) | sum d2
//   PlanePair (30): open3d's TransformationEstimationPointToPlane, no pivots.  m = the matched reference point's normal,
//       e = p - q,   r = (e0*m0 + e1*m1) + e2*m2
//       c = p x m:   c0 = p1*m2 - p2*m1,  c1 = p2*m0 - p0*m2,  c2 = p0*m1 - p1*m0,      J = (c0, c1, c2, m0, m1, m2)
//       n | sum J_i J_j for i <= j (21, the upper triangle row-major) | sum J_i r (6) | sum r^2 | sum d2
//     Negating a normal negates J and r exactly and leaves every term's bits as they are: the reference's _fix_normal_direction
//     has no effect on this aligner and is not ported.  The normals are float planes in pool memory (x, y, z, each
//     count(reference) long), gathered by idx like the reference's coordinates (IcpNormals: direction_normals of
//     kernels_direction.hip writes them once per run, before the grid hook -- open3d's KDTreeSearchParamHybrid(radius, max_nn)
//     estimate -- or the caller's are copied there).  Only the reference cloud has normals: open3d's estimate never reads the
//     source's.
//   GicpPair (30): the 30 terms of gicp_terms.hpp (gicp_pair_terms: the arithmetic and its order are stated there, the C contract
//     in include/cwipc_util_amd/hip_ext.h), in PlanePair's layout: n | sum (A^T N A)_ij (21) | sum (A^T g)_i (6) | sum e^T g |
//     sum d2.  Both clouds have covariances, made once per run from their normals (gicp_covariance_kernel): six planes for the
//     source, loaded once per four points, and records of six doubles for the reference, gathered by idx.
//   DistortionPair (10): no aligner, a measure (cwipc_hip_distortion, RULE Q of hip_ext.h): the 10 terms of quality_terms.hpp
//       n | n_plane | sum d2 | sum r^2 | sum dR^2, dG^2, dB^2 | sum dY^2, dU^2, dV^2
//     T is the identity.  The source's four colour words are one 16-byte load per step, the reference's word and the normal are
//     gathered by index.  The normals are those of the ORIGINAL cloud, whichever side it is on: the normal's index is idx itself
//     (the original is the reference) or normal_of[idx] (the original is the source: normal_of is the other pass's idx array), and
//     it is checked against the original's count before it is an address; a pair whose index fails the test has no normal.
//     This Pair also has a MAXIMUM (HAS_MAX): the largest d2 over the matched pairs.  d2 >= 0, so its bit pattern orders as an
//     unsigned 64-bit integer; a lane keeps the largest pattern of its points, shuffles close the wave, lane 0 of the workgroup takes
//     the largest of the four waves into one more slot of the chunk's row, and the final kernel reduces that slot by maximum into
//     the word behind the sums (0 without a pair).  A maximum is order-free: no atomics here either.
//
// 3. THE LOOP (icp_loop) is open3d's registration_icp: evaluate (search, sums, wait, read), then up to max_iteration times: the
// update U from the sums, T = U T, evaluate; fitness = n / count(source) and inlier_rmse = sqrt(sum d2 / n) (the point distances,
// for every aligner) after each evaluation; it stops when both change by less than the criteria.  It runs inside ONE GridSearch
// hook, so the grid over the reference is built once per run.  T is applied to the ORIGINAL float32 source points on every
// iteration (open3d moves an f64 copy step by step).  The updates: rigid_fit.hpp (umeyama without scaling, with the pivot
// cp = T cp0 that follows the cloud) for point-to-point; plane_fit.hpp (A x = -b with A the 21 sums, b the 6) for the other two.
//
// The entry points at the bottom take arguments that their caller has checked (registration.cpp: the C entry points check every scalar
// argument, once); what depends on a cloud's size is checked here (the caller's normals), and so are the pivots of icp_sums.
#include "point_grid.hpp"
#include "rigid_fit.hpp"
#include "plane_fit.hpp"
#include "gicp_terms.hpp"
#include "quality_terms.hpp"

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
    walk_exact(rows, q, c, limit, scan);
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

// ---- the sums (the scheme is stated at the top of the file) ----
constexpr size_t ICP_CHUNK = 1024;        // source points per chunk before the shift (four per lane and step)
constexpr size_t ICP_MAX_CHUNKS = 1024;
constexpr int ICP_FINAL_THREADS = 64;

// What every sums kernel is given; a Pair's Args add what its terms need.
struct IcpSumBase {
    const float *sx, *sy, *sz;   // source planes (padded to a multiple of 256 points: a lane's four points are one 16-byte load)
    size_t ns;
    const uint32_t *idx;         // the search's results, arrays padded to a multiple of 4 entries
    const double *d2;
    const float *rx, *ry, *rz;   // the reference cloud's planes, in the original order idx refers to
    size_t nr;
    double T[12];
    size_t chunk;
};

// A Pair: NSUM (the count and its sums); the launches' names; Args; Step, what step() loads once per four points of a lane
// (point u of the four is the one terms() is asked about); terms(), which writes t[1 .. NSUM - 1] for the source point moved to p
// and matched with reference point i at squared distance d2; HAS_MAX, whether the largest d2 is kept next to the sums.
struct PointPair {
    static constexpr int NSUM = 17;           // n, sum a, sum b, sum a b^T, sum d2
    static constexpr bool HAS_MAX = false;
    static constexpr const char *PARTIAL = "icp_sums_partial", *FINAL = "icp_sums_final";
    struct Args : IcpSumBase { double cp[3], cq[3]; };
    struct Step {};
    static __device__ __forceinline__ void step(const Args &, size_t, Step &) {}
    static __device__ __forceinline__ void terms(const Args &A, const Step &, int, const double (&p)[3], uint32_t i, double d2, double (&t)[NSUM]) {
        const double a[3] = {p[0] - A.cp[0], p[1] - A.cp[1], p[2] - A.cp[2]};
        const double b[3] = {(double)A.rx[i] - A.cq[0], (double)A.ry[i] - A.cq[1], (double)A.rz[i] - A.cq[2]};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            t[1 + k] = a[k];
            t[4 + k] = b[k];
#pragma unroll
            for (int j = 0; j < 3; j++) t[7 + 3 * k + j] = a[k] * b[j];
        }
        t[16] = d2;
    }
};

struct PlanePair {
    static constexpr int NSUM = 30;           // n, sum J J^T (21), sum J r (6), sum r^2, sum d2
    static constexpr bool HAS_MAX = false;
    static constexpr const char *PARTIAL = "icp_plane_sums_partial", *FINAL = "icp_plane_sums_final";
    struct Args : IcpSumBase { const float *mx, *my, *mz; };   // the reference's normals' planes, in the order of its points
    struct Step {};
    static __device__ __forceinline__ void step(const Args &, size_t, Step &) {}
    static __device__ __forceinline__ void terms(const Args &A, const Step &, int, const double (&p)[3], uint32_t i, double d2, double (&t)[NSUM]) {
        const double q[3] = {(double)A.rx[i], (double)A.ry[i], (double)A.rz[i]};
        const double m[3] = {(double)A.mx[i], (double)A.my[i], (double)A.mz[i]};
        const double e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
        const double r = (e[0] * m[0] + e[1] * m[1]) + e[2] * m[2];
        const double J[6] = {p[1] * m[2] - p[2] * m[1], p[2] * m[0] - p[0] * m[2], p[0] * m[1] - p[1] * m[0], m[0], m[1], m[2]};
#pragma unroll
        for (int k = 0; k < 6; k++)
#pragma unroll
            for (int j = k; j < 6; j++) t[1 + (k * (11 - k)) / 2 + j] = J[k] * J[j];   // (row k of the triangle begins at k (13 - k) / 2)
#pragma unroll
        for (int k = 0; k < 6; k++) t[22 + k] = J[k] * r;
        t[28] = r * r;
        t[29] = d2;
    }
};

struct GicpPair {
    static constexpr int NSUM = GICP_NTERM;
    static constexpr bool HAS_MAX = false;
    static constexpr const char *PARTIAL = "icp_gicp_sums_partial", *FINAL = "icp_plane_sums_final";
    struct Args : IcpSumBase {
        const double *cs;        // the source's covariances: six planes of cs_stride doubles (cs_stride a multiple of 256)
        size_t cs_stride;
        const double *ct;        // the reference's: nr records of six doubles
    };
    struct Step { double cs[4][6]; };   // the four source points' covariances
    static __device__ __forceinline__ void step(const Args &A, size_t base, Step &S) {
#pragma unroll
        for (int v = 0; v < 6; v++) {
            const double2 ca = *reinterpret_cast<const double2 *>(A.cs + (size_t)v * A.cs_stride + base),
                          cb = *reinterpret_cast<const double2 *>(A.cs + (size_t)v * A.cs_stride + base + 2);
            S.cs[0][v] = ca.x; S.cs[1][v] = ca.y; S.cs[2][v] = cb.x; S.cs[3][v] = cb.y;
        }
    }
    static __device__ __forceinline__ void terms(const Args &A, const Step &S, int u, const double (&p)[3], uint32_t i, double d2, double (&t)[NSUM]) {
        const double R[9] = {A.T[0], A.T[1], A.T[2], A.T[4], A.T[5], A.T[6], A.T[8], A.T[9], A.T[10]};
        const double q[3] = {(double)A.rx[i], (double)A.ry[i], (double)A.rz[i]};
        const double2 *rec = reinterpret_cast<const double2 *>(A.ct + 6 * (size_t)i);
        const double2 c0 = rec[0], c1 = rec[1], c2 = rec[2];
        const double ct[6] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y};
        gicp_pair_terms(p, q, S.cs[u], ct, R, d2, t);   // (t[0] is 1: the skeleton counts)
    }
};
static_assert(GicpPair::NSUM == PlanePair::NSUM, "the generalized sums have the plane sums' layout: one update, one set of pinned words");

struct DistortionPair {
    static constexpr int NSUM = QUALITY_NTERM;   // n, n_plane, sum d2, sum r^2, sum dRGB^2 (3), sum dYUV^2 (3)
    static constexpr bool HAS_MAX = true;        // ... and max d2
    static constexpr const char *PARTIAL = "distortion_sums_partial", *FINAL = "distortion_sums_final";
    struct Args : IcpSumBase {
        const uint32_t *srgbt, *rrgbt;   // the colour words of the source (padded like its planes) and of the reference
        const float *mx, *my, *mz;       // the ORIGINAL cloud's normals' planes, in the order of its points; nullptr: no pair has a normal
        size_t na;                       // the original's count: what a normal's index is checked against
        const uint32_t *normal_of;       // nullptr: the normal's index is idx; else normal_of[idx] (nr entries: the other pass's idx)
    };
    struct Step { uint32_t c[4]; };      // the four source points' colour words
    static __device__ __forceinline__ void step(const Args &A, size_t base, Step &S) {
        const uint4 c4 = *reinterpret_cast<const uint4 *>(A.srgbt + base);
        S.c[0] = c4.x; S.c[1] = c4.y; S.c[2] = c4.z; S.c[3] = c4.w;
    }
    static __device__ __forceinline__ void terms(const Args &A, const Step &S, int u, const double (&p)[3], uint32_t i, double d2, double (&t)[NSUM]) {
        const double q[3] = {(double)A.rx[i], (double)A.ry[i], (double)A.rz[i]};
        double m[3] = {0.0, 0.0, 0.0};
        bool has_normal = false;
        if (A.mx != nullptr) {
            // (i is below nr: the skeleton has checked it; the normal's index is checked against the original's count here)
            const size_t j = A.normal_of ? (size_t)A.normal_of[i] : (size_t)i;
            if (j < A.na) {
                m[0] = (double)A.mx[j]; m[1] = (double)A.my[j]; m[2] = (double)A.mz[j];
                has_normal = true;
            }
        }
        quality_pair_terms(p, q, m, has_normal, S.c[u], A.rrgbt[i], d2, t);   // (t[0] is 1: the skeleton counts)
    }
};
static_assert(DistortionPair::NSUM + 2 <= 32, "the 10 sums, the maximum and the tag fit the 32 pinned words of a thread");

// a chunk's row in `partial`: the NSUM sums and, for a Pair with a maximum, its bit pattern behind them
template <class Pair>
constexpr int icp_row() { return Pair::NSUM + (Pair::HAS_MAX ? 1 : 0); }

template <class Pair>
__global__ void __launch_bounds__(GRID_BLK) icp_sums_partial_kernel(typename Pair::Args A, double *__restrict__ partial /* [chunks][icp_row<Pair>()] */) {
    constexpr int NSUM = Pair::NSUM, ROW = icp_row<Pair>();
    __shared__ double red[GRID_BLK / 64][NSUM];
    const size_t lo = (size_t)blockIdx.x * A.chunk, hi = lo + A.chunk < A.ns ? lo + A.chunk : A.ns;
    double s[NSUM];
    unsigned long long largest = 0ull;   // HAS_MAX: the bit pattern of the largest d2 of this lane's matched pairs (+0.0: none)
#pragma unroll
    for (int v = 0; v < NSUM; v++) s[v] = 0.0;
    // (chunk is a multiple of 4 * GRID_BLK: a lane's points are the same whatever the launch looks like)
    for (size_t base = lo + 4 * (size_t)threadIdx.x; base < hi; base += 4 * (size_t)GRID_BLK) {
        const float4 x4 = *reinterpret_cast<const float4 *>(A.sx + base), y4 = *reinterpret_cast<const float4 *>(A.sy + base),
                     z4 = *reinterpret_cast<const float4 *>(A.sz + base);
        const uint4 i4 = *reinterpret_cast<const uint4 *>(A.idx + base);
        const double2 da = *reinterpret_cast<const double2 *>(A.d2 + base), db = *reinterpret_cast<const double2 *>(A.d2 + base + 2);
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
        const uint32_t is[4] = {i4.x, i4.y, i4.z, i4.w};
        const double ds[4] = {da.x, da.y, db.x, db.y};
        typename Pair::Step step;
        Pair::step(A, base, step);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            // (idx is checked against the reference count before it is an address; ICP_NONE fails the test too)
            if (base + u >= hi || (size_t)is[u] >= A.nr) continue;
            double p[3], t[NSUM];
            icp_move(A.T, xs[u], ys[u], zs[u], p);
            Pair::terms(A, step, u, p, is[u], ds[u], t);
            s[0] += 1.0;   // (a count below 2^53 is exact in f64)
#pragma unroll
            for (int v = 1; v < NSUM; v++) s[v] += t[v];
            if constexpr (Pair::HAS_MAX) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(ds[u]);   // (d2 >= 0: the pattern orders as the value)
                largest = bits > largest ? bits : largest;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < NSUM; v++) {
        for (int off = 32; off > 0; off >>= 1) s[v] += __shfl_down(s[v], off, 64);   // (kept: a call changed this kernel)
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][v] = s[v];
    }
    if constexpr (Pair::HAS_MAX) {
        __shared__ unsigned long long red_largest[GRID_BLK / 64];
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_down(largest, off, 64);
            largest = other > largest ? other : largest;
        }
        if ((threadIdx.x & 63) == 0) red_largest[threadIdx.x >> 6] = largest;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long t = 0ull;
            for (int w = 0; w < GRID_BLK / 64; w++) t = red_largest[w] > t ? red_largest[w] : t;
            partial[(size_t)blockIdx.x * ROW + NSUM] = __longlong_as_double((long long)t);   // (stored, never computed with)
        }
    } else {
        __syncthreads();
    }
    if (threadIdx.x < NSUM) {
        double t = 0.0;
        for (int w = 0; w < GRID_BLK / 64; w++) t += red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * ROW + threadIdx.x] = t;
    }
}

// out: NSUM + 1 pinned 64-bit words -- n as an integer, the NSUM - 1 sums, the tag; with a maximum NSUM + 2 -- its bit pattern goes
// between the sums and the tag.  `partial` has rows of NSUM + (HAS_MAX ? 1 : 0) values.
template <int NSUM, bool HAS_MAX>
__global__ void __launch_bounds__(ICP_FINAL_THREADS) icp_sums_final_kernel(const double *__restrict__ partial, size_t nchunks, unsigned long long *__restrict__ out,
                                                                          unsigned long long tag) {
    constexpr int ROW = NSUM + (HAS_MAX ? 1 : 0);
    static_assert(ROW <= ICP_FINAL_THREADS, "one lane per value");
    const int v = threadIdx.x;
    if (v >= ROW) return;
    if (HAS_MAX && v == NSUM) {
        unsigned long long largest = 0ull;
        for (size_t c = 0; c < nchunks; c++) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(partial[c * ROW + v]);
            largest = bits > largest ? bits : largest;
        }
        out[v] = largest;
        return;
    }
    double acc = 0.0;
    for (size_t c = 0; c < nchunks; c++) acc += partial[c * ROW + v];
    if (v == 0) {
        out[0] = (unsigned long long)acc;
        out[ROW] = tag;
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
    bool alloc(size_t ns, int nsum) {   // nsum: values per chunk in `partial`
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

// the two sums kernels behind a search on stream s; S holds what is the Pair's own; the result lands in the thread's pinned words under `tag`
template <class Pair>
void launch_sums(typename Pair::Args S, const DeviceSoA &source, const DeviceSoA &reference, const double T[16], const IcpWork &w, ThreadCtx &c,
                 uint32_t tag, hipStream_t s) {
    S.sx = source.x(); S.sy = source.y(); S.sz = source.z();
    S.ns = source.npoints;
    S.idx = w.idx;
    S.d2 = w.d2;
    S.rx = reference.x(); S.ry = reference.y(); S.rz = reference.z();
    S.nr = reference.npoints;
    for (int i = 0; i < 12; i++) S.T[i] = T[i];
    S.chunk = w.chunk;
    CW_LAUNCH(Pair::PARTIAL, (icp_sums_partial_kernel<Pair>), dim3((unsigned)w.nchunks), dim3(GRID_BLK), 0, s, S, w.partial);
    CW_LAUNCH(Pair::FINAL, (icp_sums_final_kernel<Pair::NSUM, Pair::HAS_MAX>), dim3(1), dim3(ICP_FINAL_THREADS), 0, s, w.partial, w.nchunks,
              c.report().device(), (unsigned long long)tag);
}

PointPair::Args point_args(const double cp[3], const double cq[3]) {
    PointPair::Args S{};
    for (int a = 0; a < 3; a++) { S.cp[a] = cp[a]; S.cq[a] = cq[a]; }
    return S;
}

PlanePair::Args plane_args(const float *normals, size_t nr) {
    PlanePair::Args S{};
    S.mx = normals; S.my = normals + nr; S.mz = normals + 2 * nr;
    return S;
}

// after a wait on the stream: the pinned words into n and the nsum - 1 sums
bool read_sums(ThreadCtx &c, uint32_t tag, int nsum, uint64_t *n, double *sums) {
    const PinnedReport report = c.report();
    if (!report.landed_plain(tag, nsum)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_icp", nsum == PointPair::NSUM ? "the sums kernel did not report" : "the plane sums kernel did not report");
        return false;
    }
    *n = report.raw(0);
    for (int v = 0; v < nsum - 1; v++) {
        const unsigned long long bits = report.raw(1 + v);
        memcpy(&sums[v], &bits, sizeof(double));
    }
    return true;
}

uint32_t next_tag(ThreadCtx &c, int nsum) {
    return c.report().arm(nsum, 1);   // (the word behind the nsum values is the tag's)
}

// The reference cloud's normals as three planes of count(reference) floats in one pool block (and, behind them, the three doubles
// direction_normals wants for its centroid): the caller's, copied, or estimated there.  On the calling thread's stream, no wait.
struct IcpNormals {
    float *planes = nullptr;
    // (checked: the caller has looked at host_normals already)
    bool make(const char *who, const DeviceSoA &reference, const float *host_normals, float radius, int max_nn, ThreadCtx &c, bool checked = false) {
        const size_t nr = reference.npoints;
        const size_t cen_at = (3 * nr * sizeof(float) + 127) & ~(size_t)127;
        planes = (float *)pool_alloc(cen_at + 3 * sizeof(double));
        if (!planes) return false;
        if (host_normals) {
            for (size_t i = 0; !checked && i < 3 * nr; i++)
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

GicpPair::Args gicp_args(const GicpClouds &g) {
    GicpPair::Args S{};
    S.cs = g.cs.values;
    S.cs_stride = g.cs.stride;
    S.ct = g.ct.values;
    return S;
}

// An aligner to the code below: the sums kernels that follow a search, put on the stream for the matrix T under `tag`, and the
// update, the motion R, t from n and the sums.  sum d2 is the last sum of every layout (nsum - 2 of the nsum - 1 values).
using SumsLaunch = std::function<void(const double T[16], uint32_t tag, hipStream_t s)>;
using IcpUpdate = std::function<void(uint64_t n, const double *sums, double R[3][3], double t[3])>;

// One search and its sums in a grid hook of their own (the parity entry points); waits.
bool search_and_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, const IcpWork &w, ThreadCtx &c, int nsum,
                     const SumsLaunch &launch, uint64_t *n, double *sums) {
    const IcpArgs A = correspond_args(source, T, max_distance, w);
    const uint32_t tag = next_tag(c, nsum);
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        launch_correspond(v, A, s);
        launch(T, tag, s);
        return hipGetLastError() == hipSuccess;
    };
    bool ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    ok = c.sync() && ok;
    return ok && read_sums(c, tag, nsum, n, sums);
}

// The loop (3. at the top of the file), from res.T; inside ONE grid hook; waits for its results.  res is written on success only.
bool icp_loop(const char *who, const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const IcpCriteria &k, const IcpWork &w,
              ThreadCtx &c, int nsum, const SumsLaunch &launch, const IcpUpdate &update, IcpResult &res) {
    const size_t ns = source.npoints;
    const int max_iteration = k.max_iteration;
    bool loop_ok = true;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        double T[16];
        for (int i = 0; i < 16; i++) T[i] = res.T[i];
        // one evaluation: search, sums, wait, read
        uint64_t n = 0;
        double sums[PlanePair::NSUM - 1];
        auto evaluate = [&]() {
            const IcpArgs A = correspond_args(source, T, max_distance, w);
            const uint32_t tag = next_tag(c, nsum);
            launch_correspond(v, A, s);
            launch(T, tag, s);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
            return read_sums(c, tag, nsum, &n, sums);
        };
        auto measures = [&](double &fit, double &rmse) {
            fit = n ? (double)n / (double)ns : 0.0;
            rmse = n ? sqrt(sums[nsum - 2] / (double)n) : 0.0;
        };
        if (!evaluate()) return loop_ok = false;
        double fit, rmse;
        measures(fit, rmse);
        int done = 0;
        if (n != 0) {
            for (int it = 0; it < max_iteration; it++) {
                double R[3][3], t[3];
                update(n, sums, R, t);
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
                if (fabs(fit_before - fit) < k.relative_fitness && fabs(rmse_before - rmse) < k.relative_rmse) break;
            }
        }
        for (int i = 0; i < 16; i++) res.T[i] = T[i];
        res.fitness = fit;
        res.inlier_rmse = rmse;
        res.iterations = done;
        return true;
    };
    bool ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    ok = c.sync() && ok;
    return ok && loop_ok;
}

void plane_update(uint64_t, const double *sums, double R[3][3], double t[3]) { plane_fit(sums, sums + 21, R, t); }

}  // namespace

bool icp_correspondences(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, uint32_t *idx_host,
                         double *d2_host) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t ns = source.npoints;
    if (ns == 0) return true;
    IcpWork w;
    if (!w.alloc(ns, PointPair::NSUM)) return false;
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
    *n = 0;
    for (int v = 0; v < 16; v++) sums[v] = 0.0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(cp[a]) || !std::isfinite(cq[a])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_icp_sums", "the pivots must be finite");
            return false;
        }
    const size_t ns = source.npoints;
    if (ns == 0 || reference.npoints == 0) return true;
    IcpWork w;
    if (!w.alloc(ns, PointPair::NSUM)) return false;
    const SumsLaunch launch = [&](const double T[16], uint32_t tag, hipStream_t s) {
        launch_sums<PointPair>(point_args(cp, cq), source, reference, T, w, c, tag, s);
    };
    return search_and_sums(source, reference, T, max_distance, w, c, PointPair::NSUM, launch, n, sums);
}

bool icp_point2point(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const IcpCriteria &k, const double cp0[3],
                     const double cq[3], IcpResult &res) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t ns = source.npoints;
    if (ns == 0 || reference.npoints == 0) return true;
    IcpWork w;
    if (!w.alloc(ns, PointPair::NSUM)) return false;
    // cp = T applied to the source's centroid: the pivot follows the cloud, from the launch of the sums to the update that reads them
    double cp[3];
    const SumsLaunch launch = [&](const double T[16], uint32_t tag, hipStream_t s) {
        for (int r = 0; r < 3; r++) cp[r] = ((T[4 * r] * cp0[0] + T[4 * r + 1] * cp0[1]) + T[4 * r + 2] * cp0[2]) + T[4 * r + 3];
        launch_sums<PointPair>(point_args(cp, cq), source, reference, T, w, c, tag, s);
    };
    const IcpUpdate update = [&](uint64_t n, const double *sums, double R[3][3], double t[3]) { rigid_fit(n, sums, sums + 3, sums + 6, cp, cq, R, t); };
    return icp_loop("cwipc_hip_icp_point2point", source, reference, max_distance, k, w, c, PointPair::NSUM, launch, update, res);
}

bool icp_plane_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, const float *host_normals, float radius,
                    int max_nn, uint64_t *n, double sums[29]) {
    *n = 0;
    for (int v = 0; v < 29; v++) sums[v] = 0.0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t ns = source.npoints;
    if (reference.npoints == 0) return true;
    IcpNormals normals;
    IcpWork w;
    // (the caller's normals are looked at even when there is nothing to match them with: a bad array is an error either way)
    bool ok = normals.make("cwipc_hip_icp_plane_sums", reference, host_normals, radius, max_nn, c);
    if (ok && ns != 0) ok = w.alloc(ns, PlanePair::NSUM);
    if (!ok || ns == 0) return c.sync() && ok;   // (a wait also on failure: kernels that write the blocks may still be in flight)
    const SumsLaunch launch = [&](const double T[16], uint32_t tag, hipStream_t s) {
        launch_sums<PlanePair>(plane_args(normals.planes, reference.npoints), source, reference, T, w, c, tag, s);
    };
    return search_and_sums(source, reference, T, max_distance, w, c, PlanePair::NSUM, launch, n, sums);
}

bool icp_point2plane(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const float *host_normals, float radius, int max_nn,
                     const IcpCriteria &k, IcpResult &res) {
    const char *who = "cwipc_hip_icp_point2plane";
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t ns = source.npoints;
    if (reference.npoints == 0) return true;
    IcpNormals normals;
    IcpWork w;
    // the normals, once per run and before the grid hook: direction_normals builds a grid of its own width
    bool ok = normals.make(who, reference, host_normals, radius, max_nn, c);
    if (ok && ns != 0) ok = w.alloc(ns, PlanePair::NSUM);
    if (!ok || ns == 0) return c.sync() && ok;
    const SumsLaunch launch = [&](const double T[16], uint32_t tag, hipStream_t s) {
        launch_sums<PlanePair>(plane_args(normals.planes, reference.npoints), source, reference, T, w, c, tag, s);
    };
    return icp_loop(who, source, reference, max_distance, k, w, c, PlanePair::NSUM, launch, plane_update, res);
}

bool icp_gicp_covariances(const DeviceSoA &cloud, const float *host_normals, float radius, int max_nn, const double *direction, double epsilon,
                          double *cov_host) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t n = cloud.npoints;
    if (n == 0) return true;
    IcpNormals normals;
    GicpCov cov;
    bool ok = normals.make("cwipc_hip_gicp_covariances", cloud, host_normals, radius, max_nn, c) && cov.make(cloud, normals.planes, direction, epsilon, true, c);
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
    const size_t ns = source.npoints;
    // (the caller's normals are looked at even when there is nothing to match them with: a bad array is an error either way)
    if (!normals_finite(who, source_normals, ns) || !normals_finite(who, reference_normals, reference.npoints)) return false;
    if (ns == 0 || reference.npoints == 0) return true;
    GicpClouds clouds;
    IcpWork w;
    const bool ok = clouds.make(who, source, reference, source_normals, reference_normals, radius, max_nn, epsilon, c) && w.alloc(ns, GicpPair::NSUM);
    if (!ok) return c.sync() && ok;   // (a wait also on failure: kernels that write the blocks may still be in flight)
    const SumsLaunch launch = [&](const double T[16], uint32_t tag, hipStream_t s) {
        launch_sums<GicpPair>(gicp_args(clouds), source, reference, T, w, c, tag, s);
    };
    return search_and_sums(source, reference, T, max_distance, w, c, GicpPair::NSUM, launch, n, sums);
}

bool icp_generalized(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const float *source_normals,
                     const float *reference_normals, float radius, int max_nn, double epsilon, const IcpCriteria &k, IcpResult &res) {
    const char *who = "cwipc_hip_icp_generalized";
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t ns = source.npoints;
    if (!normals_finite(who, source_normals, ns) || !normals_finite(who, reference_normals, reference.npoints)) return false;
    if (ns == 0 || reference.npoints == 0) return true;
    GicpClouds clouds;
    IcpWork w;
    const bool ok = clouds.make(who, source, reference, source_normals, reference_normals, radius, max_nn, epsilon, c) && w.alloc(ns, GicpPair::NSUM);
    if (!ok) return c.sync() && ok;
    const SumsLaunch launch = [&](const double T[16], uint32_t tag, hipStream_t s) {
        launch_sums<GicpPair>(gicp_args(clouds), source, reference, T, w, c, tag, s);
    };
    return icp_loop(who, source, reference, max_distance, k, w, c, GicpPair::NSUM, launch, plane_update, res);
}

namespace {

// One pass of cwipc_hip_distortion in a grid hook of its own: the grid over the pass's reference, the search (T the identity), the
// two sums kernels; waits, and reads the 10 sums and the maximum from the pinned words.  normal_planes: the original's (nullptr: no
// normals), na its count, normal_of: see DistortionPair.
bool distortion_pass(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const float *normal_planes, size_t na,
                     const uint32_t *normal_of, const IcpWork &w, ThreadCtx &c, cwipc_hip_distortion_sums &out) {
    constexpr int NV = icp_row<DistortionPair>();   // the values in front of the tag
    static const double identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    DistortionPair::Args S{};
    S.srgbt = source.rgbt();
    S.rrgbt = reference.rgbt();
    S.mx = normal_planes;
    S.my = normal_planes ? normal_planes + na : nullptr;
    S.mz = normal_planes ? normal_planes + 2 * na : nullptr;
    S.na = na;
    S.normal_of = normal_of;
    const IcpArgs A = correspond_args(source, identity, max_distance, w);
    const uint32_t tag = next_tag(c, NV);
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        launch_correspond(v, A, s);
        launch_sums<DistortionPair>(S, source, reference, identity, w, c, tag, s);
        return hipGetLastError() == hipSuccess;
    };
    bool ok = grid_and_search(reference, ICP_GRID_WIDTH, true, search);
    ok = c.sync() && ok;   // (also on failure: kernels that write the block may still be in flight)
    if (!ok) return false;
    const PinnedReport report = c.report();
    if (!report.landed_plain(tag, NV)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_distortion", "the sums kernel did not report");
        return false;
    }
    auto as_double = [&](int i) {
        const unsigned long long bits = report.raw(i);
        double v;
        memcpy(&v, &bits, sizeof(v));
        return v;
    };
    out.n = report.raw(0);
    // (the counts and the three RGB sums are sums of integers below 2^53: exact in f64 in any order)
    out.n_plane = (uint64_t)as_double(1);
    out.sum_d2 = as_double(2);
    out.sum_r2 = as_double(3);
    for (int k = 0; k < 3; k++) {
        out.sum_rgb2[k] = (uint64_t)as_double(4 + k);
        out.sum_yuv2[k] = as_double(7 + k);
    }
    out.max_d2 = as_double(DistortionPair::NSUM);
    return true;
}

}  // namespace

bool icp_distortion(const DeviceSoA &original, const DeviceSoA &degraded, double max_distance, const float *host_normals, float radius, int max_nn,
                    bool plane, cwipc_hip_distortion_sums out[2]) {
    const char *who = "cwipc_hip_distortion";
    const size_t na = original.npoints, nb = degraded.npoints;
    memset(out, 0, 2 * sizeof(out[0]));
    out[0].n_source = na;
    out[1].n_source = nb;
    if (na == 0 || nb == 0) return true;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    IcpNormals normals;
    IcpWork backward, forward;
    // the original's normals, once per call and before the grid hooks: direction_normals builds a grid of its own width
    bool ok = !plane || normals.make(who, original, host_normals, radius, max_nn, c, true);
    ok = ok && backward.alloc(nb, icp_row<DistortionPair>()) && forward.alloc(na, icp_row<DistortionPair>());
    if (!ok) return c.sync() && ok;   // (a wait also on failure: kernels that write the blocks may still be in flight)
    // backward: source the degraded cloud, reference the original; its idx array stays on the device and hands the forward pass,
    // whose reference is the degraded cloud, the original's normals
    return distortion_pass(degraded, original, max_distance, normals.planes, na, nullptr, backward, c, out[1]) &&
           distortion_pass(original, degraded, max_distance, normals.planes, na, backward.idx, forward, c, out[0]);
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
