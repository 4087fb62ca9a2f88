// smooth_terms.hpp -- the per-point arithmetic of cwipc_hip_smooth (RULE N of include/cwipc_util_amd/hip_ext.h has the contract in
// full): a neighbour's quantised offset and weight, the ten integer sums, the move decision and the step from the sums to the
// displacement.  Host- and device-compilable, like gicp_terms.hpp and quality_terms.hpp: neigh_smooth_kernel (kernels_neigh.hip)
// includes it for the device, cwipc_hip_smooth_host (filters.cpp) and a stand-alone host program (tests/abi/smooth_host.cpp, built
// with the sanitizers by tests/test_smooth_host.py) compile the same text with the host compiler, and tests/neigh_model.py is its
// numpy model.  Every f64 operation is rounded on its own (-ffp-contract=off); the order written here is the contract.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "smallest_eigvec.hpp"

namespace cwipc_amd {

constexpr double SMOOTH_FIX = 65536.0;        // fixed-point units per radius: |o_a| <= 65536
constexpr double SMOOTH_WEIGHT = 4096.0;      // the weight of a neighbour at distance 0
constexpr uint64_t SMOOTH_MAX_CNT = 262144;   // a term is at most 2^44: the 64-bit sums are exact up to 2^18 neighbours

// radius finite and within [1e-30, 1e30]: r2 and 65536 / radius are finite, normal numbers
CWIPC_HOST_DEVICE inline bool smooth_radius_ok(double radius) { return radius >= 1e-30 && radius <= 1e30; }

// The sums over N(i), i itself included.  64-bit words with wrapping arithmetic (unsigned here; read as two's complement).
struct SmoothSums {
    uint64_t W = 0, S1[3] = {0, 0, 0}, S2[6] = {0, 0, 0, 0, 0, 0};   // S2: xx xy xz yy yz zz
    uint64_t cnt = 0;
};

// d2 of RULE N (RULE K's): d_a = (double)p_j[a] - (double)p_i[a]
CWIPC_HOST_DEVICE inline double smooth_d2(const double (&d)[3]) { return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]; }

// One neighbour (d2 < r2 has been tested) into the sums.  |o_a| <= 65536 and w <= 4096, so o_a, w and w * o_a fit 32 bits and every
// product below is one 32 x 32 -> 64 bit multiply-add (v_mad_i64_i32 on the device) of values that cannot overflow.
CWIPC_HOST_DEVICE inline void smooth_add(SmoothSums &S, const double (&d)[3], double d2, double r2, double s) {
    const int32_t o0 = (int32_t)rint(d[0] * s), o1 = (int32_t)rint(d[1] * s), o2 = (int32_t)rint(d[2] * s);
    const double t = 1.0 - d2 / r2;
    const int32_t w = (int32_t)rint(SMOOTH_WEIGHT * (t * t));
    const int32_t w0 = w * o0, w1 = w * o1, w2 = w * o2;
    S.cnt++;
    S.W += (uint64_t)(int64_t)w;
    S.S1[0] += (uint64_t)(int64_t)w0;
    S.S1[1] += (uint64_t)(int64_t)w1;
    S.S1[2] += (uint64_t)(int64_t)w2;
    S.S2[0] += (uint64_t)((int64_t)w0 * (int64_t)o0);
    S.S2[1] += (uint64_t)((int64_t)w0 * (int64_t)o1);
    S.S2[2] += (uint64_t)((int64_t)w0 * (int64_t)o2);
    S.S2[3] += (uint64_t)((int64_t)w1 * (int64_t)o1);
    S.S2[4] += (uint64_t)((int64_t)w1 * (int64_t)o2);
    S.S2[5] += (uint64_t)((int64_t)w2 * (int64_t)o2);
}

// The move decision for a finite point with cnt = |N(i)|
CWIPC_HOST_DEVICE inline bool smooth_moves(uint64_t cnt, uint32_t min_neighbours) {
    const uint64_t need = min_neighbours > 2u ? (uint64_t)min_neighbours : 2u;
    return cnt >= 1u && cnt - 1u >= need && cnt <= SMOOTH_MAX_CNT;
}

// From the sums of a moved point to its displacement in the cloud's units: (n * (n . c)) / s, n the normal of the weighted
// covariance, c the weighted mean offset.  The sign of n cancels.
CWIPC_HOST_DEVICE inline void smooth_displacement(const SmoothSums &S, double s, double (&disp)[3]) {
    const double W = (double)(int64_t)S.W;
    const double s1[3] = {(double)(int64_t)S.S1[0], (double)(int64_t)S.S1[1], (double)(int64_t)S.S1[2]};
    double M[3][3];
    M[0][0] = W * (double)(int64_t)S.S2[0] - s1[0] * s1[0];
    M[0][1] = M[1][0] = W * (double)(int64_t)S.S2[1] - s1[0] * s1[1];
    M[0][2] = M[2][0] = W * (double)(int64_t)S.S2[2] - s1[0] * s1[2];
    M[1][1] = W * (double)(int64_t)S.S2[3] - s1[1] * s1[1];
    M[1][2] = M[2][1] = W * (double)(int64_t)S.S2[4] - s1[1] * s1[2];
    M[2][2] = W * (double)(int64_t)S.S2[5] - s1[2] * s1[2];
    double n[3];
    smallest_eigvec(M, n);
    const double c[3] = {s1[0] / W, s1[1] / W, s1[2] / W};
    const double h = (n[0] * c[0] + n[1] * c[1]) + n[2] * c[2];
    for (int a = 0; a < 3; a++) disp[a] = (n[a] * h) / s;
}

// The host twin of neigh_smooth_kernel: brute force over all pairs, O(n * n).  P is a cwipc_point (x, y, z floats, then r, g, b and
// the tile byte); out may not alias pts.  Host code only.
template <class P>
inline void smooth_brute_force(const P *pts, size_t n, double radius, bool same_tile, uint32_t min_neighbours, P *out) {
    const double r2 = radius * radius, s = SMOOTH_FIX / radius;
    for (size_t i = 0; i < n; i++) {
        out[i] = pts[i];
        const P &me = pts[i];
        if (!(std::isfinite(me.x) && std::isfinite(me.y) && std::isfinite(me.z))) continue;
        SmoothSums S;
        for (size_t j = 0; j < n; j++) {
            const P &p = pts[j];
            const double d[3] = {(double)p.x - (double)me.x, (double)p.y - (double)me.y, (double)p.z - (double)me.z};
            const double d2 = smooth_d2(d);
            if (!(d2 < r2)) continue;   // (a non-finite coordinate: inf or NaN, never under the limit)
            if (same_tile && p.tile != me.tile) continue;
            smooth_add(S, d, d2, r2, s);
        }
        if (!smooth_moves(S.cnt, min_neighbours)) continue;
        double disp[3];
        smooth_displacement(S, s, disp);
        out[i].x = (float)((double)me.x + disp[0]);
        out[i].y = (float)((double)me.y + disp[1]);
        out[i].z = (float)((double)me.z + disp[2]);
    }
}

}  // namespace cwipc_amd
