// plane_seg_terms.hpp -- the per-hypothesis and per-point arithmetic of plane segmentation (RULE S of include/cwipc_util_amd/hip_ext.h
// has the contract in full): the draw of a triple, the plane through it, the signed distance and the inlier test, the refit's
// quantised offsets and integer sums, and -- host only -- the exact refit matrix, its solve, the orientation and the levelling
// motion.  No HIP type.  The kernels (kernels_plane.hip, the plane classifier of kernels_floor.hip) include it for the device;
// cwipc_hip_plane_find, cwipc_hip_plane_find_host (registration.cpp) and a stand-alone host program (tests/abi/plane_seg_host.cpp, built
// with the sanitizers by tests/test_plane_seg_host.py) compile the same text with the host compiler; tests/plane_model.py is its numpy
// model.  (plane_fit.hpp is something else: the 6x6 solve of point-to-plane ICP.)
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "counter_rng.hpp"
#include "smallest_eigvec.hpp"

namespace cwipc_amd {

constexpr unsigned long long RNG_TAG_PLANE = 0x706c616e65ull;   // "plane"
constexpr uint32_t PLANE_MAX_ITERATIONS = 65536;
constexpr double PLANE_FIX = 16.0;               // fixed-point units per distance
constexpr double PLANE_MAX_OFFSET = 262144.0;    // |o_a| <= 2^18: a product is at most 2^36, the sums are exact up to 2^26 inliers
constexpr uint64_t PLANE_MAX_CNT = 1ull << 26;

CWIPC_HOST_DEVICE inline bool plane_distance_ok(double distance) { return distance >= 1e-30 && distance <= 1e30; }

// What the caller hands over (cwipc_hip_plane_params without the C types)
struct PlaneRule {
    double distance;
    double axis[3];
    double min_abs_cos;
    unsigned long long base;   // rng_base(seed, RNG_TAG_PLANE)
    uint32_t iterations;
    bool constrained;          // min_abs_cos > 0 and a non-zero axis
};

CWIPC_HOST_DEVICE inline bool plane_rule_ok(double distance, uint32_t iterations, const double axis[3], double min_abs_cos) {
    if (!plane_distance_ok(distance) || iterations < 1 || iterations > PLANE_MAX_ITERATIONS) return false;
    if (!(min_abs_cos >= 0.0 && min_abs_cos <= 1.0)) return false;
    for (int a = 0; a < 3; a++)
        if (!(fabs(axis[a]) <= 1e30)) return false;   // (finite; a unit axis is the caller's business)
    return true;
}

CWIPC_HOST_DEVICE inline PlaneRule plane_rule(double distance, uint32_t iterations, unsigned long long seed, const double axis[3], double min_abs_cos) {
    PlaneRule r;
    r.distance = distance;
    r.iterations = iterations;
    r.base = rng_base(seed, RNG_TAG_PLANE);
    r.min_abs_cos = min_abs_cos;
    for (int a = 0; a < 3; a++) r.axis[a] = axis[a];
    r.constrained = min_abs_cos > 0.0 && (axis[0] != 0.0 || axis[1] != 0.0 || axis[2] != 0.0);
    return r;
}

// (n_x a_x + n_y a_y) + n_z a_z
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double plane_dot(const double n[3], const double a[3]) {
    return rn_add(rn_add(rn_mul(n[0], a[0]), rn_mul(n[1], a[1])), rn_mul(n[2], a[2]));
}

// the point indices of hypothesis h in a cloud of n < 2^32 points
CWIPC_HOST_DEVICE inline void plane_triple(unsigned long long base, uint32_t h, unsigned long long n, uint32_t idx[3]) {
    for (int k = 0; k < 3; k++) {
        const unsigned long long x = rng_draw(base, 3ull * h + (unsigned long long)k);
        idx[k] = (uint32_t)(((x >> 32) * n) >> 32);
    }
}

CWIPC_HOST_DEVICE inline bool plane_triple_distinct(const uint32_t idx[3]) { return idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2]; }

CWIPC_HOST_DEVICE inline bool plane_constraint_holds(const PlaneRule &r, const double n[3]) {
    return !r.constrained || fabs(plane_dot(n, r.axis)) >= r.min_abs_cos;   // (a NaN fails)
}

// The plane through three points whose indices differ; plane = n_x, n_y, n_z, d.  False (plane = four +0.0): the hypothesis is invalid.
CWIPC_HOST_DEVICE inline bool plane_through(const PlaneRule &r, const double p0[3], const double p1[3], const double p2[3], double plane[4]) {
    plane[0] = plane[1] = plane[2] = plane[3] = 0.0;
    for (int a = 0; a < 3; a++)
        if (!(std::isfinite(p0[a]) && std::isfinite(p1[a]) && std::isfinite(p2[a]))) return false;
    double u[3], v[3];
    for (int a = 0; a < 3; a++) { u[a] = rn_add(p1[a], -p0[a]); v[a] = rn_add(p2[a], -p0[a]); }
    const double c[3] = {rn_add(rn_mul(u[1], v[2]), -rn_mul(u[2], v[1])), rn_add(rn_mul(u[2], v[0]), -rn_mul(u[0], v[2])),
                         rn_add(rn_mul(u[0], v[1]), -rn_mul(u[1], v[0]))};
    const double l2 = rn_add(rn_add(rn_mul(c[0], c[0]), rn_mul(c[1], c[1])), rn_mul(c[2], c[2]));
    if (!(std::isfinite(l2) && l2 > 0.0)) return false;
    const double len = rn_sqrt(l2);
    const double n[3] = {rn_div(c[0], len), rn_div(c[1], len), rn_div(c[2], len)};
    if (!plane_constraint_holds(r, n)) return false;
    plane[0] = n[0]; plane[1] = n[1]; plane[2] = n[2];
    plane[3] = -plane_dot(n, p0);
    return true;
}

// e(p) = ((n_x x + n_y y) + n_z z) + d
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double plane_e(const double plane[4], double x, double y, double z) {
    return rn_add(rn_add(rn_add(rn_mul(plane[0], x), rn_mul(plane[1], y)), rn_mul(plane[2], z)), plane[3]);
}
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool plane_inlier(double e, double distance) { return fabs(e) <= distance; }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool plane_below(double e, double distance) { return e <= distance; }

// An inlier's quantised offsets from the anchor; false: it takes no part (an offset beyond 2^18 units, or not a number).
CWIPC_HOST_DEVICE inline bool plane_offsets(const double p[3], const double anchor[3], double s, int64_t o[3]) {
    bool ok = true;
    for (int a = 0; a < 3; a++) {
        const double q = rint(rn_mul(rn_add(p[a], -anchor[a]), s));
        ok = ok && fabs(q) <= PLANE_MAX_OFFSET;
        o[a] = ok ? (int64_t)q : 0;
    }
    return ok;
}

// The refit's sums v: cnt, S1[3], S2[6] (xx xy xz yy yz zz).  64-bit words with wrapping arithmetic, read as two's complement.
CWIPC_HOST_DEVICE inline void plane_sums_add(uint64_t v[10], const int64_t o[3]) {
    v[0] += 1u;
    v[1] += (uint64_t)o[0]; v[2] += (uint64_t)o[1]; v[3] += (uint64_t)o[2];
    v[4] += (uint64_t)(o[0] * o[0]); v[5] += (uint64_t)(o[0] * o[1]); v[6] += (uint64_t)(o[0] * o[2]);
    v[7] += (uint64_t)(o[1] * o[1]); v[8] += (uint64_t)(o[1] * o[2]); v[9] += (uint64_t)(o[2] * o[2]);
}

// ---------------------------------------------------------------------------
// host only from here on (plain functions: 128-bit integers and long double stay off the device)
// ---------------------------------------------------------------------------

// M_ab = cnt * S2_ab - S1_a * S1_b exactly, rounded to double once (xx xy xz yy yz zz).  cnt <= 2^26: |cnt * S2| <= 2^114.
inline void plane_refit_matrix(const uint64_t v[10], double M6[6]) {
    const __int128 cnt = (__int128)(int64_t)v[0];
    const __int128 s1[3] = {(__int128)(int64_t)v[1], (__int128)(int64_t)v[2], (__int128)(int64_t)v[3]};
    static const int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
    for (int i = 0; i < 6; i++) M6[i] = (double)(cnt * (__int128)(int64_t)v[4 + i] - s1[A[i]] * s1[B[i]]);
}

// The refit's plane from the sums (3 <= cnt <= 2^26 is the caller's check).  False: n' is not finite or misses the constraint.
inline bool plane_refit_solve(const PlaneRule &r, const uint64_t v[10], const double anchor[3], const double hyp[4], double M6[6], double out[4]) {
    plane_refit_matrix(v, M6);
    double M[3][3] = {{M6[0], M6[1], M6[2]}, {M6[1], M6[3], M6[4]}, {M6[2], M6[4], M6[5]}};
    double n[3];
    smallest_eigvec(M, n);
    out[0] = out[1] = out[2] = out[3] = 0.0;
    if (!(std::isfinite(n[0]) && std::isfinite(n[1]) && std::isfinite(n[2]))) return false;
    if (!(plane_dot(n, hyp) >= 0.0))
        for (int a = 0; a < 3; a++) n[a] = -n[a];
    if (!plane_constraint_holds(r, n)) return false;
    const double s = rn_div(PLANE_FIX, r.distance), cnt = (double)(int64_t)v[0];
    double c[3];
    for (int a = 0; a < 3; a++) c[a] = rn_add(anchor[a], rn_div(rn_div((double)(int64_t)v[1 + a], cnt), s));
    out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
    out[3] = -plane_dot(n, c);
    return true;
}

// The returned plane's orientation: negated iff n . a < 0, a the caller's axis or (0, 1, 0) when unconstrained.
inline void plane_orient(const PlaneRule &r, double plane[4]) {
    const double up[3] = {0.0, 1.0, 0.0};
    if (plane_dot(plane, r.constrained ? r.axis : up) < 0.0)
        for (int a = 0; a < 4; a++) plane[a] = -plane[a];
}

// Levelling: the row-major 4x4 of the minimal rotation taking n to (0, 1, 0), t = (0, d, 0).  False: a non-finite plane or a zero normal.
inline bool plane_level_matrix(const double plane[4], double m16[16]) {
    typedef long double ld;
    for (int a = 0; a < 4; a++)
        if (!std::isfinite(plane[a])) return false;
    const ld sign = plane[1] < 0.0 ? -1.0L : 1.0L;
    const ld len = sqrtl((ld)plane[0] * plane[0] + (ld)plane[1] * plane[1] + (ld)plane[2] * plane[2]);
    if (!(len > 0.0L) || !std::isfinite((double)len)) return false;
    const ld nx = sign * plane[0] / len, ny = sign * plane[1] / len, nz = sign * plane[2] / len, d = sign * plane[3] / len;
    const ld f = 1.0L / (1.0L + ny);
    const double m[16] = {(double)(1.0L - f * nx * nx), (double)-nx, (double)(-f * nx * nz), 0.0,
                          (double)nx, (double)ny, (double)nz, (double)d,
                          (double)(-f * nx * nz), (double)-nz, (double)(1.0L - f * nz * nz), 0.0,
                          0.0, 0.0, 0.0, 1.0};
    for (int i = 0; i < 16; i++) m16[i] = m[i];
    return true;
}

// What a search leaves behind, in the layout of cwipc_hip_plane_result
struct PlaneFound {
    double plane[4] = {0, 0, 0, 0}, hypothesis[4] = {0, 0, 0, 0};
    uint64_t sums[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double M[6] = {0, 0, 0, 0, 0, 0};
    uint32_t best = 0, triple[3] = {0, 0, 0}, count = 0, recount = 0, valid = 0;
    int32_t found = 0, refined = 0;
};

// After best and sums are known: solve, and say whether a recount is wanted (`refit` then holds the plane to count).
inline bool plane_refit_wanted(const PlaneRule &r, PlaneFound &f, const double anchor[3], double refit[4]) {
    const uint64_t cnt = f.sums[0];
    if (!f.found || cnt < 3 || cnt > PLANE_MAX_CNT) return false;
    return plane_refit_solve(r, f.sums, anchor, f.hypothesis, f.M, refit);
}

// ... and after the recount: which plane is returned, oriented.
inline void plane_conclude(const PlaneRule &r, PlaneFound &f, bool recounted, const double refit[4], uint32_t recount) {
    if (!f.found) return;
    f.recount = recounted ? recount : 0;
    f.refined = recounted && recount >= f.count ? 1 : 0;
    for (int a = 0; a < 4; a++) f.plane[a] = f.refined ? refit[a] : f.hypothesis[a];
    plane_orient(r, f.plane);
}

// The host twin of the kernels: brute force.  P is a cwipc_point.  planes (4 H), counts (H), valid (H) may be null.
template <class P>
inline void plane_find_brute(const P *pts, size_t n, const PlaneRule &r, bool refine, PlaneFound &f, double *planes, uint32_t *counts, uint8_t *valid) {
    f = PlaneFound();
    bool any = false;
    double best_anchor[3] = {0, 0, 0};
    auto count_of = [&](const double plane[4]) {
        uint32_t c = 0;
        for (size_t i = 0; i < n; i++) c += plane_inlier(plane_e(plane, (double)pts[i].x, (double)pts[i].y, (double)pts[i].z), r.distance) ? 1u : 0u;
        return c;
    };
    for (uint32_t h = 0; h < r.iterations; h++) {
        uint32_t idx[3];
        plane_triple(r.base, h, n, idx);
        double plane[4] = {0, 0, 0, 0}, p[3][3];
        bool ok = plane_triple_distinct(idx);
        if (ok) {
            for (int k = 0; k < 3; k++) { p[k][0] = (double)pts[idx[k]].x; p[k][1] = (double)pts[idx[k]].y; p[k][2] = (double)pts[idx[k]].z; }
            ok = plane_through(r, p[0], p[1], p[2], plane);
        }
        const uint32_t c = ok ? count_of(plane) : 0;
        if (planes) for (int a = 0; a < 4; a++) planes[4 * (size_t)h + a] = plane[a];
        if (counts) counts[h] = c;
        if (valid) valid[h] = ok ? 1 : 0;
        if (!ok) continue;
        f.valid++;
        if (!any || c > f.count) {
            any = true;
            f.found = 1; f.best = h; f.count = c;
            for (int a = 0; a < 4; a++) f.hypothesis[a] = plane[a];
            for (int k = 0; k < 3; k++) { f.triple[k] = idx[k]; best_anchor[k] = p[0][k]; }
        }
    }
    if (!f.found) return;
    double refit[4] = {0, 0, 0, 0};
    bool recounted = false;
    uint32_t recount = 0;
    if (refine) {
        const double s = rn_div(PLANE_FIX, r.distance);
        for (size_t i = 0; i < n; i++) {
            const double q[3] = {(double)pts[i].x, (double)pts[i].y, (double)pts[i].z};
            if (!plane_inlier(plane_e(f.hypothesis, q[0], q[1], q[2]), r.distance)) continue;
            int64_t o[3];
            if (plane_offsets(q, best_anchor, s, o)) plane_sums_add(f.sums, o);
        }
        recounted = plane_refit_wanted(r, f, best_anchor, refit);
        if (recounted) recount = count_of(refit);
    }
    plane_conclude(r, f, recounted, refit, recount);
}

}  // namespace cwipc_amd
