// registration.cpp -- C entry points of the registration tooling and their host orchestration: nearest-neighbour distances and
// their jobs, the kernel density estimate, every ICP and GICP entry, the distortion measure, the floor and tile helpers, bounds.  The per-point work is in
// kernels_nn.hip, kernels_kde.hip, kernels_icp.hip and kernels_floor.hip.  There is NO CPU fallback.
#include "entry.hpp"
#include "plane_seg_terms.hpp"

#include <cmath>
#include <cstring>

using namespace cwipc_amd;

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/analyze.py:116-123 (the KD-tree query) and :171-179 (gaussian_kde)
// ---------------------------------------------------------------------------
extern "C" int cwipc_hip_nn_distance2(cwipc_pointcloud *source, cwipc_pointcloud *reference, int nth, double max_distance, double *dist2, size_t cap) {
    const char *who = "cwipc_hip_nn_distance2";
    if (source == nullptr || reference == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return -1;
    }
    if (nth < 0 || nth > NN_MAX_NTH || !(max_distance > 0.0)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "nth must lie between 0 and 31, max_distance must be positive (inf: no bound)");
        return -1;
    }
    std::unique_ptr<cwipc_hip_pointcloud> keep_src, keep_ref;
    auto src = device_input(who, source, keep_src);
    if (!src) return -1;
    auto ref = source == reference ? src : device_input(who, reference, keep_ref);
    if (!ref) return -1;
    const size_t n = src->npoints;
    if (cap < n || (n && dist2 == nullptr)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the result array is too small");
        return -1;
    }
    if (n == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    double *dev = (double *)pool_alloc(n * sizeof(double));
    if (!dev) return -1;
    bool ok = nn_distance2(*src, *ref, nth, max_distance, dev);
    ok = ok && hipMemcpyAsync(dist2, dev, n * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;   // (also on failure: kernels that write `dev` may still be in flight)
    pool_free(dev);
    return ok ? 0 : -1;
}

extern "C" int cwipc_hip_nn_distance2_jobs(cwipc_pointcloud *source, cwipc_pointcloud *reference, const cwipc_hip_nn_job *jobs, int njobs, double *dist2,
                                           size_t cap) {
    const char *who = "cwipc_hip_nn_distance2_jobs";
    if (source == nullptr || reference == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return -1;
    }
    if (jobs == nullptr || njobs < 1 || njobs > NN_MAX_JOBS) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "between 1 and 64 jobs");
        return -1;
    }
    for (int j = 0; j < njobs; j++) {
        const cwipc_hip_nn_job &b = jobs[j];
        if (b.nth < 0 || b.nth > NN_MAX_NTH || !(b.max_distance > 0.0) || std::isnan(b.source_y[0]) || std::isnan(b.source_y[1]) ||
            std::isnan(b.reference_y[0]) || std::isnan(b.reference_y[1])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "nth must lie between 0 and 31, max_distance must be positive (inf: no bound), a y limit is not NaN");
            return -1;
        }
    }
    std::unique_ptr<cwipc_hip_pointcloud> keep_src, keep_ref;
    auto src = device_input(who, source, keep_src);
    if (!src) return -1;
    auto ref = source == reference ? src : device_input(who, reference, keep_ref);
    if (!ref) return -1;
    const size_t n = src->npoints;
    if (cap < n || (n && dist2 == nullptr)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the result array is too small");
        return -1;
    }
    if (n == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    double *dev = (double *)pool_alloc((size_t)njobs * n * sizeof(double));
    void *table = pool_alloc(nn_jobs_table_bytes(njobs));
    if (!dev || !table) { pool_free(dev); pool_free(table); return -1; }
    bool ok = nn_distance2_jobs(*src, *ref, jobs, njobs, dev, table);
    if (ok && cap == n) {
        ok = hipMemcpyAsync(dist2, dev, (size_t)njobs * n * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    } else {
        for (int j = 0; ok && j < njobs; j++)
            ok = hipMemcpyAsync(dist2 + (size_t)j * cap, dev + (size_t)j * n, n * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    }
    ok = c.sync() && ok;   // (also on failure: kernels that read the table and write `dev` may still be in flight)
    pool_free(dev);
    pool_free(table);
    return ok ? 0 : -1;
}

extern "C" int cwipc_hip_gaussian_kde(const double *samples, size_t n, double h, const double *at, size_t m, double *density) {
    const char *who = "cwipc_hip_gaussian_kde";
    if (n == 0 || samples == nullptr || !(h > 0.0) || !std::isfinite(h) || (m && (at == nullptr || density == nullptr))) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "needs at least one sample, a positive, finite bandwidth and arrays for the evaluation points");
        return -1;
    }
    if (m == 0) return 0;
    if (!device_available(who)) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    // one block: samples | evaluation points | densities
    double *block = (double *)pool_alloc((n + 2 * m) * sizeof(double));
    if (!block) return -1;
    double *ds = block, *da = block + n, *dd = block + n + m;
    bool ok = hipMemcpyAsync(ds, samples, n * sizeof(double), hipMemcpyHostToDevice, c.stream) == hipSuccess &&
              hipMemcpyAsync(da, at, m * sizeof(double), hipMemcpyHostToDevice, c.stream) == hipSuccess;
    ok = ok && gaussian_kde(ds, n, h, da, m, dd);
    ok = ok && hipMemcpyAsync(density, dd, m * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(block);
    return ok ? 0 : -1;
}

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/fine.py (open3d registration_icp) and analyze.py's OverlapAnalyzer (evaluate_registration):
// kernels_icp.hip
// ---------------------------------------------------------------------------
namespace {

const double ICP_IDENTITY[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// The scalar arguments of the ICP entry points are checked HERE, once (kernels_icp.hip takes them as checked), in the order of the
// helpers below; false: logged.
struct IcpClouds {
    std::unique_ptr<cwipc_hip_pointcloud> keep_src, keep_ref;
    std::shared_ptr<DeviceSoA> src, ref;
};

// both clouds on the device, and the arguments every ICP entry point has
bool icp_inputs(const char *who, cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance, IcpClouds &in) {
    if (source == nullptr || reference == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return false;
    }
    if (!(max_distance > 0.0)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_distance must be positive (inf: no bound)");
        return false;
    }
    for (int i = 0; T && i < 16; i++)
        if (!std::isfinite(T[i])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the matrix must be finite");
            return false;
        }
    in.src = device_input(who, source, in.keep_src);
    if (!in.src) return false;
    in.ref = source == reference ? in.src : device_input(who, reference, in.keep_ref);
    return (bool)in.ref;
}

bool icp_criteria_ok(const char *who, const IcpCriteria &k) {
    if (k.max_iteration >= 0 && !std::isnan(k.relative_fitness) && !std::isnan(k.relative_rmse)) return true;
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_iteration must not be negative, the criteria not NaN");
    return false;
}

bool gicp_epsilon_ok(const char *who, double epsilon) {
    if (epsilon > 0.0 && std::isfinite(epsilon)) return true;
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "epsilon must be positive and finite");
    return false;
}

// an entry point's body between the C caller and C++: 0 / -1, no exception leaves
template <class Body>
int icp_entry(const char *who, Body &&body) {
    try {
        return body() ? 0 : -1;
    } catch (...) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "exception");
        return -1;
    }
}

// What an aligner starts from, which is also what its caller gets when it fails; and a result into the caller's optional pointers.
IcpResult icp_start(const double *init) {
    IcpResult r{};
    memcpy(r.T, init ? init : ICP_IDENTITY, sizeof(r.T));
    return r;
}

void icp_result_out(const IcpResult &r, double *T_out, double *fitness, double *inlier_rmse, int *iterations) {
    if (T_out) memcpy(T_out, r.T, sizeof(r.T));
    if (fitness) *fitness = r.fitness;
    if (inlier_rmse) *inlier_rmse = r.inlier_rmse;
    if (iterations) *iterations = r.iterations;
}

void icp_sums_out(uint64_t hn, const double *hs, int count, uint64_t *n, double *sums) {
    if (n) *n = hn;
    if (sums) memcpy(sums, hs, (size_t)count * sizeof(double));
}

}  // namespace

extern "C" int cwipc_hip_correspondences(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance, uint32_t *idx,
                                         double *dist2, size_t cap) {
    const char *who = "cwipc_hip_correspondences";
    return icp_entry(who, [&] {
        IcpClouds in;
        if (!icp_inputs(who, source, reference, T, max_distance, in)) return false;
        const size_t n = in.src->npoints;
        if (cap < n) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the result arrays are too small");
            return false;
        }
        return n == 0 || icp_correspondences(*in.src, *in.ref, T ? T : ICP_IDENTITY, max_distance, idx, dist2);
    });
}

extern "C" int cwipc_hip_icp_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance, const double *cp,
                                  const double *cq, uint64_t *n, double *sums) {
    const char *who = "cwipc_hip_icp_sums";
    uint64_t hn = 0;
    double hs[16] = {};
    icp_sums_out(hn, hs, 16, n, sums);
    return icp_entry(who, [&] {
        IcpClouds in;
        if (!icp_inputs(who, source, reference, T, max_distance, in)) return false;
        const double zero[3] = {0, 0, 0};
        if (!icp_sums(*in.src, *in.ref, T ? T : ICP_IDENTITY, max_distance, cp ? cp : zero, cq ? cq : zero, &hn, hs)) return false;
        icp_sums_out(hn, hs, 16, n, sums);
        return true;
    });
}

extern "C" int cwipc_hip_icp_point2point(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init,
                                         double relative_fitness, double relative_rmse, int max_iteration, double *T_out, double *fitness,
                                         double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_point2point";
    IcpResult res = icp_start(init);
    icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
    return icp_entry(who, [&] {
        IcpClouds in;
        const IcpCriteria k{relative_fitness, relative_rmse, max_iteration};
        if (!icp_inputs(who, source, reference, init, max_distance, in) || !icp_criteria_ok(who, k)) return false;
        if (in.src->npoints == 0 || in.ref->npoints == 0) return true;
        // the pivots, once per run: the clouds' centroids ((0, 0, 0) for a cloud with a non-finite point: any pivot is right,
        // a near one only keeps the covariance from cancelling)
        double cp0[3], cq[3];
        if (!icp_centroid(*in.src, cp0) || !icp_centroid(*in.ref, cq)) return false;
        if (!(std::isfinite(cp0[0]) && std::isfinite(cp0[1]) && std::isfinite(cp0[2]))) cp0[0] = cp0[1] = cp0[2] = 0.0;
        if (!(std::isfinite(cq[0]) && std::isfinite(cq[1]) && std::isfinite(cq[2]))) cq[0] = cq[1] = cq[2] = 0.0;
        if (!icp_point2point(*in.src, *in.ref, max_distance, k, cp0, cq, res)) return false;
        icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
        return true;
    });
}

extern "C" int cwipc_hip_icp_plane_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance, const float *normals,
                                        float radius, int max_nn, uint64_t *n, double *sums) {
    const char *who = "cwipc_hip_icp_plane_sums";
    uint64_t hn = 0;
    double hs[29] = {};
    icp_sums_out(hn, hs, 29, n, sums);
    return icp_entry(who, [&] {
        IcpClouds in;
        if (!icp_inputs(who, source, reference, T, max_distance, in)) return false;
        if (!normals && !direction_args_ok(who, radius, max_nn)) return false;
        if (!icp_plane_sums(*in.src, *in.ref, T ? T : ICP_IDENTITY, max_distance, normals, radius, max_nn, &hn, hs)) return false;
        icp_sums_out(hn, hs, 29, n, sums);
        return true;
    });
}

extern "C" int cwipc_hip_icp_point2plane(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init, const float *normals,
                                         float radius, int max_nn, double relative_fitness, double relative_rmse, int max_iteration, double *T_out,
                                         double *fitness, double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_point2plane";
    IcpResult res = icp_start(init);
    icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
    return icp_entry(who, [&] {
        IcpClouds in;
        const IcpCriteria k{relative_fitness, relative_rmse, max_iteration};
        if (!icp_inputs(who, source, reference, init, max_distance, in)) return false;
        if (!normals && !direction_args_ok(who, radius, max_nn)) return false;
        if (!icp_criteria_ok(who, k)) return false;
        if (!icp_point2plane(*in.src, *in.ref, max_distance, normals, radius, max_nn, k, res)) return false;
        icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
        return true;
    });
}

extern "C" int cwipc_hip_gicp_covariances(cwipc_pointcloud *pc, const float *normals, float radius, int max_nn, const double *direction, double epsilon,
                                          double *cov, size_t cap) {
    const char *who = "cwipc_hip_gicp_covariances";
    return icp_entry(who, [&] {
        if (pc == nullptr) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
            return false;
        }
        if (!gicp_epsilon_ok(who, epsilon)) return false;
        if (!normals && !direction_args_ok(who, radius, max_nn)) return false;
        std::unique_ptr<cwipc_hip_pointcloud> keep;
        auto src = device_input(who, pc, keep);
        if (!src) return false;
        const size_t n = src->npoints;
        if (cap < n || (n && cov == nullptr)) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the result array is too small");
            return false;
        }
        return icp_gicp_covariances(*src, normals, radius, max_nn, direction, epsilon, cov);
    });
}

extern "C" int cwipc_hip_icp_gicp_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance,
                                       const float *source_normals, const float *reference_normals, float radius, int max_nn, double epsilon, uint64_t *n,
                                       double *sums) {
    const char *who = "cwipc_hip_icp_gicp_sums";
    uint64_t hn = 0;
    double hs[29] = {};
    icp_sums_out(hn, hs, 29, n, sums);
    return icp_entry(who, [&] {
        IcpClouds in;
        if (!icp_inputs(who, source, reference, T, max_distance, in)) return false;
        if (!(source_normals && reference_normals) && !direction_args_ok(who, radius, max_nn)) return false;
        if (!gicp_epsilon_ok(who, epsilon)) return false;
        if (!icp_gicp_sums(*in.src, *in.ref, T ? T : ICP_IDENTITY, max_distance, source_normals, reference_normals, radius, max_nn, epsilon, &hn, hs)) return false;
        icp_sums_out(hn, hs, 29, n, sums);
        return true;
    });
}

extern "C" int cwipc_hip_icp_generalized(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init,
                                         const float *source_normals, const float *reference_normals, float radius, int max_nn, double epsilon,
                                         double relative_fitness, double relative_rmse, int max_iteration, double *T_out, double *fitness,
                                         double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_generalized";
    IcpResult res = icp_start(init);
    icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
    return icp_entry(who, [&] {
        IcpClouds in;
        const IcpCriteria k{relative_fitness, relative_rmse, max_iteration};
        if (!icp_inputs(who, source, reference, init, max_distance, in)) return false;
        if (!(source_normals && reference_normals) && !direction_args_ok(who, radius, max_nn)) return false;
        if (!gicp_epsilon_ok(who, epsilon) || !icp_criteria_ok(who, k)) return false;
        if (!icp_generalized(*in.src, *in.ref, max_distance, source_normals, reference_normals, radius, max_nn, epsilon, k, res)) return false;
        icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
        return true;
    });
}

// ---------------------------------------------------------------------------
// no reference counterpart: the distortion of a degraded cloud against its original (RULE Q of hip_ext.h; DistortionPair of
// kernels_icp.hip, quality_terms.hpp)
// ---------------------------------------------------------------------------
extern "C" int cwipc_hip_distortion(cwipc_pointcloud *original, cwipc_pointcloud *degraded, double max_distance, const float *normals, float radius,
                                    int max_nn, int flags, cwipc_hip_distortion_sums out[2]) {
    const char *who = "cwipc_hip_distortion";
    if (out) memset(out, 0, 2 * sizeof(out[0]));
    return icp_entry(who, [&] {
        if (out == nullptr) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL result");
            return false;
        }
        if ((flags & ~CWIPC_HIP_DISTORTION_NO_PLANE) != 0) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "unknown flag");
            return false;
        }
        const bool plane = (flags & CWIPC_HIP_DISTORTION_NO_PLANE) == 0;
        if (original == nullptr || degraded == nullptr) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
            return false;
        }
        if (!(max_distance > 0.0)) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_distance must be positive (inf: no bound)");
            return false;
        }
        if (plane && !normals && !direction_args_ok(who, radius, max_nn)) return false;
        // (before either cloud is brought to the device: a refused call launches and allocates nothing)
        for (size_t i = 0, n3 = 3 * (size_t)original->count(); plane && normals && i < n3; i++)
            if (!std::isfinite(normals[i])) {
                cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the normals must be finite");
                return false;
            }
        IcpClouds in;
        if (!icp_inputs(who, original, degraded, nullptr, max_distance, in)) return false;
        cwipc_hip_distortion_sums sums[2];
        if (!icp_distortion(*in.src, *in.ref, max_distance, normals, radius, max_nn, plane, sums)) return false;
        memcpy(out, sums, sizeof(sums));
        return true;
    });
}

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/util.py:146-229: the floor and tile helpers (kernels_floor.hip)
// ---------------------------------------------------------------------------
namespace {

// count -> scan -> (wait: the two totals size the result) -> scatter -> wait.  Args: k::FloorArgs, or k::PlaneArgs for RULE S's classes.
template <class Args>
std::shared_ptr<DeviceSoA> floor_partition(const std::shared_ptr<DeviceSoA> &src, const Args &a, uint64_t *n_first) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    if (n_first) *n_first = 0;
    const size_t n = src->npoints;
    if (n == 0) return soa_alloc(0);
    const size_t nb = k::floor_blocks(n);
    uint32_t *counts = (uint32_t *)c.device_scratch((2 * nb + 2) * sizeof(uint32_t));
    if (!counts) return nullptr;
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 2);
    k::floor_count(*src, a, counts, c.stream);
    k::floor_scan(counts, nb, report.device(), tag, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = c.sync() && ok;
    if (!ok || !report.landed(tag, 0, 2)) {
        hip_failed(hipGetLastError(), "floor partition", __FILE__, __LINE__);
        return nullptr;
    }
    const size_t na = report.value(0), nrest = report.value(1);
    if (na + nrest > n) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip", "floor partition: inconsistent count");
        return nullptr;
    }
    if (n_first) *n_first = na;
    if (na == n || nrest == n) {
        // one class holds every point: the result is the input, point for point -- it holds the input's planes (clouds are immutable)
        auto same = share_planes(*src);
        same->set_tiles_from(*src);
        return same;
    }
    auto dst = soa_alloc(na + nrest);
    if (!dst) return nullptr;
    if (na + nrest) {
        k::floor_scatter(*src, a, counts, *dst, c.stream);
        ok = hipGetLastError() == hipSuccess;
        ok = c.sync() && ok;
        if (!ok) { hip_failed(hipGetLastError(), "floor partition", __FILE__, __LINE__); return nullptr; }
    }
    dst->set_tiles_from(*src);   // (a subset of the points: what could not occur still cannot)
    return dst;
}

}  // namespace

extern "C" cwipc_pointcloud *cwipc_hip_floor_partition(cwipc_pointcloud *pc, double level, int flags, double radius, uint64_t *n_first) {
    if (n_first) *n_first = 0;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_floor_partition", pc, keep);
    if (!src) return nullptr;
    // (cellsize 0: the reference builds its result with cwipc_from_numpy_matrix and does not copy the cellsize, util.py:154, :228)
    return wrap(floor_partition(src, k::FloorArgs{level, radius, flags}, n_first), pc->timestamp(), 0.f);
}

extern "C" cwipc_pointcloud *cwipc_hip_randomize_floor(cwipc_pointcloud *pc, double level, uint64_t seed) {
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_randomize_floor", pc, keep);
    if (!src) return nullptr;
    uint64_t n_first = 0;
    auto parted = floor_partition(src, k::FloorArgs{level, 0.0, k::FLOOR_KEEP_FLOOR | k::FLOOR_KEEP_REST}, &n_first);
    if (!parted) return nullptr;
    if (n_first < 2) return wrap(parted, pc->timestamp(), 0.f);   // nothing to permute
    ThreadCtx &c = tctx();
    auto dst = soa_with_new_rgbt(parted);   // the coordinates do not change: the result holds the very same planes
    if (!dst) return nullptr;
    bool ok = k::floor_shuffle(parted->rgbt(), (size_t)n_first, parted->npoints, seed, dst->rgbt(), c.stream);
    ok = ok && hipGetLastError() == hipSuccess;
    ok = c.sync() && ok;
    if (!ok) return nullptr;
    dst->set_tiles_from(*parted);   // (the same tile bytes in another order)
    return wrap(dst, pc->timestamp(), 0.f);
}

extern "C" int cwipc_hip_floor_radius_stats(cwipc_pointcloud *pc, double level, uint64_t count[2], float stat[4]) {
    if (count) count[0] = count[1] = 0;
    if (stat) for (int i = 0; i < 4; i++) stat[i] = NAN;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_floor_radius_stats", pc, keep);
    if (!src || count == nullptr || stat == nullptr) return -1;
    if (src->npoints == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    uint32_t *state = (uint32_t *)pool_alloc(k::floor_radius_state_bytes());
    if (!state) return -1;
    k::floor_radius_select(*src, level, state, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(c.host_words, state, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;   // (also on failure: kernels that write `state` may still be in flight)
    pool_free(state);
    if (!ok) return -1;
    count[0] = c.host_words[0];
    count[1] = c.host_words[1];
    memcpy(stat, c.host_words + 2, 4 * sizeof(float));
    return 0;
}

extern "C" int cwipc_hip_tile_counts(cwipc_pointcloud *pc, int nonfloor_only, double level, uint64_t counts[256]) {
    if (counts) memset(counts, 0, 256 * sizeof(uint64_t));
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_tile_counts", pc, keep);
    if (!src || counts == nullptr) return -1;
    if (src->npoints == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    unsigned long long *dev = (unsigned long long *)pool_alloc(256 * sizeof(unsigned long long));
    void *stage = c.staging(256 * sizeof(unsigned long long));
    if (!dev || !stage) { pool_free(dev); return -1; }
    k::tile_histogram(*src, nonfloor_only ? 1 : 0, level, dev, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(stage, dev, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(dev);
    if (!ok) return -1;
    memcpy(counts, stage, 256 * sizeof(uint64_t));
    return 0;
}

extern "C" int cwipc_hip_bounds(cwipc_pointcloud *pc, float minmax[6]) {
    if (minmax) for (int a = 0; a < 3; a++) { minmax[a] = INFINITY; minmax[3 + a] = -INFINITY; }
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_bounds", pc, keep);
    if (!src || minmax == nullptr) return -1;
    if (src->npoints == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const unsigned nb = k::bounds_blocks(src->npoints);
    const size_t bytes = (size_t)nb * 6 * sizeof(float);
    float *partial = (float *)pool_alloc(bytes);
    float *host = (float *)c.staging(bytes);
    if (!partial || !host) { pool_free(partial); return -1; }
    k::bounds_partial(*src, partial, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(host, partial, bytes, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(partial);
    if (!ok) return -1;
    for (unsigned b = 0; b < nb; b++)
        for (int a = 0; a < 3; a++) {
            minmax[a] = fminf(minmax[a], host[b * 6 + a]);
            minmax[3 + a] = fmaxf(minmax[3 + a], host[b * 6 + 3 + a]);
        }
    return 0;
}

// ---------------------------------------------------------------------------
// no reference counterpart: plane segmentation (RULE S of hip_ext.h; kernels_plane.hip, the plane classifier of kernels_floor.hip,
// plane_seg_terms.hpp) -- the entry of a cloud whose floor is not yet at y = 0 into the helpers above
// ---------------------------------------------------------------------------
namespace {

// The refusals of RULE S that concern the parameters; `r` and `refine` are set when they pass.
bool plane_params_refused(const char *who, const cwipc_hip_plane_params *p, PlaneRule &r, bool &refine) {
    if (p == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL parameters");
        return true;
    }
    if ((p->flags & ~CWIPC_HIP_PLANE_REFINE) != 0) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "unknown flag bits");
        return true;
    }
    if (!plane_rule_ok(p->distance, p->iterations, p->axis, p->min_abs_cos)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "distance must be finite and within [1e-30, 1e30], iterations in 1 .. 65536, min_abs_cos in [0, 1], the axis finite");
        return true;
    }
    r = plane_rule(p->distance, p->iterations, p->seed, p->axis, p->min_abs_cos);
    refine = (p->flags & CWIPC_HIP_PLANE_REFINE) != 0;
    return false;
}

bool plane_given_refused(const char *who, const double plane[4], double distance) {
    if (plane == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL plane");
        return true;
    }
    bool finite = true;
    for (int a = 0; a < 4; a++) finite = finite && std::isfinite(plane[a]);
    if (!finite || (plane[0] == 0.0 && plane[1] == 0.0 && plane[2] == 0.0)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the plane must be finite and its normal not zero");
        return true;
    }
    if (!plane_distance_ok(distance)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "distance must be finite and within [1e-30, 1e30]");
        return true;
    }
    return false;
}

void plane_result_out(const PlaneFound &f, cwipc_hip_plane_result *out) {
    memset(out, 0, sizeof(*out));
    for (int a = 0; a < 4; a++) { out->plane[a] = f.plane[a]; out->hypothesis[a] = f.hypothesis[a]; }
    for (int i = 0; i < 10; i++) out->sums[i] = (int64_t)f.sums[i];
    for (int i = 0; i < 6; i++) out->M[i] = f.M[i];
    out->best = f.best;
    for (int k = 0; k < 3; k++) out->triple[k] = f.triple[k];
    out->count = f.count; out->recount = f.recount; out->valid = f.valid;
    out->found = f.found; out->refined = f.refined;
}

// hypotheses -> score -> [best -> refit sums] -> (wait) -> [host solve -> recount -> (wait)].  table_only: no best, no refit.
bool plane_search(const char *who, const DeviceSoA &src, const PlaneRule &r, bool refine, bool table_only, PlaneFound &f, double *planes, uint32_t *counts,
                  uint32_t *triples, uint8_t *valid) {
    const size_t n = src.npoints;
    const uint32_t H = r.iterations;
    if (n >= ((size_t)1 << 32)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the cloud has 2^32 points or more");
        return false;
    }
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    void *block = pool_alloc(k::plane_work_bytes(n, H));
    if (!block) return false;
    k::PlaneWork w;
    k::plane_work_layout(block, n, H, w);
    // the read-back: the best record, then the table where it is wanted
    const bool table = planes || counts || triples || valid;
    const size_t at_planes = 256, at_counts = at_planes + (size_t)H * 32, at_triples = at_counts + (size_t)H * 4, at_valid = at_triples + (size_t)H * 12;
    char *stage = (char *)c.staging(table ? at_valid + (size_t)H * 4 : at_planes);
    if (!stage) { pool_free(block); return false; }
    static_assert(sizeof(k::PlaneBest) <= 256, "the read-back's layout");
    k::plane_hypotheses(src, r, w, c.stream);
    k::plane_score(src, r.distance, H, w, nullptr, c.stream);
    if (!table_only) {
        k::plane_best(src, H, w, c.stream);
        if (refine) k::plane_refit_sums(src, r.distance, w, c.stream);
    }
    bool ok = hipGetLastError() == hipSuccess;
    if (!table_only) ok = ok && hipMemcpyAsync(stage, w.best, sizeof(k::PlaneBest), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    if (table) {
        ok = ok && hipMemcpyAsync(stage + at_planes, w.planes, (size_t)H * 32, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(stage + at_counts, w.counts, (size_t)H * 4, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(stage + at_triples, w.triples, (size_t)H * 12, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(stage + at_valid, w.valid, (size_t)H * 4, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    }
    ok = c.sync() && ok;   // (also on failure: kernels that write the block may still be in flight)
    if (ok && table) {
        if (planes) memcpy(planes, stage + at_planes, (size_t)H * 32);
        if (counts) memcpy(counts, stage + at_counts, (size_t)H * 4);
        if (triples) memcpy(triples, stage + at_triples, (size_t)H * 12);
        const uint32_t *v = (const uint32_t *)(stage + at_valid);
        for (uint32_t h = 0; valid && h < H; h++) valid[h] = v[h] ? 1 : 0;
    }
    f = PlaneFound();
    if (ok && !table_only) {
        k::PlaneBest b;
        memcpy(&b, stage, sizeof(b));
        f.found = b.found ? 1 : 0;
        f.valid = b.nvalid;
        if (f.found) {
            f.best = b.h; f.count = b.count;
            for (int a = 0; a < 4; a++) f.hypothesis[a] = b.plane[a];
            for (int k = 0; k < 3; k++) f.triple[k] = b.triple[k];
            for (int i = 0; i < 10; i++) f.sums[i] = b.sums[i];
            double refit[4] = {0, 0, 0, 0};
            uint32_t recount = 0;
            const bool recounted = refine && plane_refit_wanted(r, f, b.anchor, refit);
            if (recounted) {
                k::plane_score(src, r.distance, H, w, refit, c.stream);
                ok = hipGetLastError() == hipSuccess;
                ok = ok && hipMemcpyAsync(stage, w.counts, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
                ok = c.sync() && ok;
                memcpy(&recount, stage, sizeof(recount));
            }
            if (ok) plane_conclude(r, f, recounted, refit, recount);
        }
    }
    pool_free(block);
    if (!ok) hip_failed(hipGetLastError(), who, __FILE__, __LINE__);
    return ok;
}

}  // namespace

extern "C" int cwipc_hip_plane_find(cwipc_pointcloud *pc, const cwipc_hip_plane_params *params, cwipc_hip_plane_result *result) {
    const char *who = "cwipc_hip_plane_find";
    if (result) memset(result, 0, sizeof(*result));
    if (pc == nullptr || result == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, pc ? "NULL result" : "NULL pointcloud");
        return -1;
    }
    PlaneRule r;
    bool refine = false;
    if (plane_params_refused(who, params, r, refine)) return -1;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input(who, pc, keep);
    if (!src) return -1;
    PlaneFound f;
    if (!plane_search(who, *src, r, refine, false, f, nullptr, nullptr, nullptr, nullptr)) return -1;
    plane_result_out(f, result);
    return 0;
}

extern "C" int cwipc_hip_plane_scores(cwipc_pointcloud *pc, const cwipc_hip_plane_params *params, double *planes, uint32_t *counts, uint32_t *triples,
                                      uint8_t *valid) {
    const char *who = "cwipc_hip_plane_scores";
    if (pc == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return -1;
    }
    PlaneRule r;
    bool refine = false;
    if (plane_params_refused(who, params, r, refine)) return -1;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input(who, pc, keep);
    if (!src) return -1;
    PlaneFound f;
    return plane_search(who, *src, r, false, true, f, planes, counts, triples, valid) ? 0 : -1;
}

extern "C" cwipc_pointcloud *cwipc_hip_plane_partition(cwipc_pointcloud *pc, const double plane[4], double distance, int flags, uint64_t *n_first) {
    const char *who = "cwipc_hip_plane_partition";
    if (n_first) *n_first = 0;
    if (pc == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return nullptr;
    }
    if ((flags & ~(CWIPC_HIP_PLANE_KEEP_INLIERS | CWIPC_HIP_PLANE_KEEP_REST | CWIPC_HIP_PLANE_BELOW_IS_INLIER)) != 0) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "unknown flag bits");
        return nullptr;
    }
    if (plane_given_refused(who, plane, distance)) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input(who, pc, keep);
    if (!src) return nullptr;
    const k::PlaneArgs a{{plane[0], plane[1], plane[2], plane[3]}, distance, flags};
    return wrap(floor_partition(src, a, n_first), pc->timestamp(), pc->cellsize());
}

extern "C" int cwipc_hip_plane_level_matrix(const double plane[4], double m16[16]) {
    const char *who = "cwipc_hip_plane_level_matrix";
    if (m16 == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL matrix");
        return -1;
    }
    if (plane_given_refused(who, plane, 1.0)) return -1;
    if (!plane_level_matrix(plane, m16)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the normal's length is not a finite positive number");
        return -1;
    }
    return 0;
}

extern "C" int cwipc_hip_plane_find_host(const cwipc_point *pts, size_t n, const cwipc_hip_plane_params *params, cwipc_hip_plane_result *result, double *planes,
                                         uint32_t *counts, uint8_t *valid) {
    const char *who = "cwipc_hip_plane_find_host";
    if (result) memset(result, 0, sizeof(*result));
    if (result == nullptr || (n && pts == nullptr)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointer");
        return -1;
    }
    PlaneRule r;
    bool refine = false;
    if (plane_params_refused(who, params, r, refine)) return -1;
    if (n >= ((size_t)1 << 32)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "2^32 points or more");
        return -1;
    }
    PlaneFound f;
    plane_find_brute(pts, n, r, refine, f, planes, counts, valid);
    plane_result_out(f, result);
    return 0;
}
