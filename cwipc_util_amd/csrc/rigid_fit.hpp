// rigid_fit.hpp -- the rigid transformation that best maps matched points onto each other, from their sums: the step of
// point-to-point ICP (kernels_icp.hip).  Host only, no HIP type: a host test (tests/test_rigid_fit_host.py, through
// tests/abi/rigid_fit_host.cpp) compiles the same text with the host C++ compiler and checks it against numpy.
//
// Eigen's umeyama without scaling (what open3d's TransformationEstimationPointToPoint calls).  With pivots cp, cq, a = p - cp,
// b = q - cq over n matched pairs (p, q):
//     mu_a = sum a / n,  mu_b = sum b / n,  Sigma = (sum b a^T - sum b (sum a)^T / n) / n
//     Sigma = U D V^T (singular values descending),  S = diag(1, 1, sign(det U * det V)),  R = U S V^T
//     t = (cq + mu_b) - R (cp + mu_a)
// The SVD is one-sided Jacobi (Hestenes): columns p, q of G = Sigma V are rotated against each other until every pair satisfies
//     |g_p . g_q| <= RIGID_FIT_TOL * |g_p| |g_q|                                  (the stopping rule; at most 30 sweeps)
// then the columns' lengths are the singular values and the columns over their lengths are U.  A column whose length is not above
// 1e-14 of the longest is taken for 0, and its place in U is filled from the others (the cross product of two columns; any unit
// vector orthogonal to the only one; the unit matrix when Sigma is 0), so that a degenerate covariance -- collinear or coincident
// pairs, n < 3 -- still gives a proper rotation: the one umeyama defines where it is unique, one of the minimisers otherwise.
//
// The bound RIGID_FIT_BOUND on every entry of R^T R - I, and on det R - 1: U's three pairs of columns are orthogonal within
// RIGID_FIT_TOL each and its columns have unit length within 3 eps; V is a product of at most 90 rotations, each orthonormal
// within 2 eps = TOL / 8: 3 + 1 + 12 < 64 times RIGID_FIT_TOL.  Against another backward stable solver R agrees within the same
// bound times the problem's condition, sigma_1 / (sigma_2 + s sigma_3) with s = sign(det U det V).
#pragma once

#include <cmath>
#include <cstdint>

namespace cwipc_amd {

constexpr double RIGID_FIT_TOL = 3.5527136788005009e-15;    // 2^-48: sixteen eps, above what rounding leaves of a rotated pair's product
constexpr double RIGID_FIT_BOUND = 64.0 * RIGID_FIT_TOL;    // 2.3e-13

namespace rigid_fit_detail {

inline double det3(const double m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

inline void cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

inline bool normalise3(double v[3]) {
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(len > 0.0)) return false;
    for (int k = 0; k < 3; k++) v[k] /= len;
    return true;
}

}  // namespace rigid_fit_detail

// sigma (3x3) = U diag(d) V^T with d descending; U and V orthonormal (U completed where d is 0)
inline void svd3(const double sigma[3][3], double U[3][3], double d[3], double V[3][3]) {
    using namespace rigid_fit_detail;
    double g[3][3];   // g[k][j]: entry k of column j
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            g[i][j] = sigma[i][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int r = 0; r < 3; r++) {
            const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2;
            double alpha = 0.0, beta = 0.0, gamma = 0.0;
            for (int k = 0; k < 3; k++) {
                alpha += g[k][p] * g[k][p];
                beta += g[k][q] * g[k][q];
                gamma += g[k][p] * g[k][q];
            }
            if (!(fabs(gamma) > RIGID_FIT_TOL * sqrt(alpha) * sqrt(beta))) continue;
            rotated = true;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; k++) {
                const double gp = g[k][p], gq = g[k][q];
                g[k][p] = c * gp - s * gq;
                g[k][q] = s * gp + c * gq;
                const double vp = V[k][p], vq = V[k][q];
                V[k][p] = c * vp - s * vq;
                V[k][q] = s * vp + c * vq;
            }
        }
        if (!rotated) break;
    }
    // columns by descending length (a stable selection: ties keep their order)
    double len[3];
    int order[3] = {0, 1, 2};
    for (int j = 0; j < 3; j++) len[j] = sqrt(g[0][j] * g[0][j] + g[1][j] * g[1][j] + g[2][j] * g[2][j]);
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2 - i; j++)
            if (len[order[j + 1]] > len[order[j]]) { const int o = order[j]; order[j] = order[j + 1]; order[j + 1] = o; }
    double Vs[3][3], u[3][3];   // u[j]: column j of U
    int rank = 0;
    for (int j = 0; j < 3; j++) {
        const int o = order[j];
        d[j] = len[o];
        for (int k = 0; k < 3; k++) Vs[k][j] = V[k][o];
        const bool nonzero = len[o] > 0.0 && len[o] > 1e-14 * len[order[0]];
        if (nonzero) {
            for (int k = 0; k < 3; k++) u[j][k] = g[k][o] / len[o];
            rank = j + 1;
        }
    }
    if (rank == 0) {
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) u[j][k] = j == k ? 1.0 : 0.0;
    } else if (rank == 1) {
        // any unit vector orthogonal to u[0]: from the axis u[0] has least of
        int m = 0;
        if (fabs(u[0][1]) < fabs(u[0][m])) m = 1;
        if (fabs(u[0][2]) < fabs(u[0][m])) m = 2;
        const double e[3] = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
        cross3(u[0], e, u[1]);
        normalise3(u[1]);
        cross3(u[0], u[1], u[2]);
        normalise3(u[2]);
    } else if (rank == 2) {
        cross3(u[0], u[1], u[2]);
        normalise3(u[2]);
    }
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) {
            U[k][j] = u[j][k];
            V[k][j] = Vs[k][j];
        }
}

// n pairs; sum_a, sum_b: 3 values each; sum_ab: 9 values, row-major a_i b_j; R and t with q ~ R p + t.  n == 0: the identity.
inline void rigid_fit(uint64_t n, const double sum_a[3], const double sum_b[3], const double sum_ab[9], const double cp[3], const double cq[3],
                      double R[3][3], double t[3]) {
    using namespace rigid_fit_detail;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = i == j ? 1.0 : 0.0;
        t[i] = 0.0;
    }
    if (n == 0) return;
    const double dn = (double)n;
    double sigma[3][3], mu_a[3], mu_b[3];
    for (int i = 0; i < 3; i++) {
        mu_a[i] = sum_a[i] / dn;
        mu_b[i] = sum_b[i] / dn;
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) sigma[i][j] = (sum_ab[3 * j + i] - sum_b[i] * sum_a[j] / dn) / dn;
    double U[3][3], d[3], V[3][3];
    svd3(sigma, U, d, V);
    const double s = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i][j] = (U[i][0] * V[j][0] + U[i][1] * V[j][1]) + s * U[i][2] * V[j][2];
    for (int i = 0; i < 3; i++) {
        const double p[3] = {cp[0] + mu_a[0], cp[1] + mu_a[1], cp[2] + mu_a[2]};
        t[i] = (cq[i] + mu_b[i]) - ((R[i][0] * p[0] + R[i][1] * p[1]) + R[i][2] * p[2]);
    }
}

}  // namespace cwipc_amd
