// plane_fit.hpp -- the update of point-to-plane ICP from its sums: a 6x6 solve and the rigid motion of its solution
// (kernels_icp.hip).  Host only, no HIP type: a host test (tests/test_plane_fit_host.py, through tests/abi/plane_fit_host.cpp)
// compiles the same text with the host C++ compiler and checks it against numpy.
//
// What open3d's TransformationEstimationPointToPlane does with J^T J and J^T r (SolveJacobianSystemAndObtainExtrinsicMatrix):
//     A = sum J J^T (6x6, given as its upper triangle, row-major: 21 values),  b = sum J r (6 values)
//     A x = -b by LDL^T with diagonal pivoting (the largest remaining diagonal entry comes next; ties: the first), in f64
//     det = the product of the pivots d
// and the update is the identity when |det| < PLANE_FIT_MIN_DET, when a pivot is <= 0, or when a pivot, det or an entry of x is
// not finite (open3d's check_det rule: a system it will not trust).  Otherwise, with x = (alpha, beta, gamma, t0, t1, t2):
//     R = Rz(gamma) Ry(beta) Rx(alpha),  t = (t0, t1, t2)                          (open3d's TransformVector6dToMatrix4d)
// A is symmetric positive semi-definite by construction; with diagonal pivoting LDL^T is Cholesky's factorisation of the permuted
// matrix, so the solve is backward stable and x is within Higham's bound 2 gamma_19 cond_2(A) |x| of the exact solution.
#pragma once

#include <cmath>

namespace cwipc_amd {

constexpr double PLANE_FIT_MIN_DET = 1e-6;

// x with A x = -b; *det = the product of the pivots taken so far.  False (x untouched) where the rule above says identity.
inline bool plane_solve6(const double A21[21], const double b[6], double x[6], double *det) {
    double a[6][6], rhs[6];
    int perm[6];
    for (int i = 0, v = 0; i < 6; i++) {
        for (int j = i; j < 6; j++, v++) a[i][j] = a[j][i] = A21[v];
        rhs[i] = -b[i];
        perm[i] = i;
    }
    *det = 1.0;
    for (int k = 0; k < 6; k++) {
        int p = k;
        for (int j = k + 1; j < 6; j++)
            if (a[j][j] > a[p][p]) p = j;
        if (p != k) {   // rows and columns k and p change places
            for (int j = 0; j < 6; j++) { const double s = a[k][j]; a[k][j] = a[p][j]; a[p][j] = s; }
            for (int i = 0; i < 6; i++) { const double s = a[i][k]; a[i][k] = a[i][p]; a[i][p] = s; }
            const double s = rhs[k]; rhs[k] = rhs[p]; rhs[p] = s;
            const int o = perm[k]; perm[k] = perm[p]; perm[p] = o;
        }
        const double d = a[k][k];
        *det *= d;
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        // column k of L goes below the diagonal (row k keeps l_j d); the rest of the matrix loses l_i d l_j
        for (int i = k + 1; i < 6; i++) {
            const double l = a[i][k] / d;
            for (int j = k + 1; j <= i; j++) a[i][j] -= l * a[k][j];
            a[i][k] = l;
        }
        for (int i = k + 1; i < 6; i++)
            for (int j = k + 1; j < i; j++) a[j][i] = a[i][j];
    }
    if (!std::isfinite(*det) || fabs(*det) < PLANE_FIT_MIN_DET) return false;
    double y[6];
    for (int i = 0; i < 6; i++) {   // L y = P rhs
        double s = rhs[i];
        for (int j = 0; j < i; j++) s -= a[i][j] * y[j];
        y[i] = s;
    }
    for (int i = 0; i < 6; i++) y[i] /= a[i][i];
    for (int i = 5; i >= 0; i--) {   // L^T z = y
        double s = y[i];
        for (int j = i + 1; j < 6; j++) s -= a[j][i] * y[j];
        y[i] = s;
    }
    for (int i = 0; i < 6; i++)
        if (!std::isfinite(y[i])) return false;
    for (int i = 0; i < 6; i++) x[perm[i]] = y[i];
    return true;
}

// R = Rz(x[2]) Ry(x[1]) Rx(x[0]), t = (x[3], x[4], x[5]).  The entries are worked out in long double and rounded once: every
// entry of R is within 2^-53 of an exactly orthonormal matrix's, so every entry of R^T R - I stays within PLANE_FIT_ORTHO_BOUND
// (in f64 alone the two- and three-factor products leave up to twice that).
constexpr double PLANE_FIT_ORTHO_BOUND = 4.0 * 1.1102230246251565e-16;   // 4 * 2^-53
inline void plane_motion(const double x[6], double R[3][3], double t[3]) {
    typedef long double ld;
    const ld sa = sinl((ld)x[0]), ca = cosl((ld)x[0]), sb = sinl((ld)x[1]), cb = cosl((ld)x[1]), sc = sinl((ld)x[2]), cc = cosl((ld)x[2]);
    R[0][0] = (double)(cc * cb);  R[0][1] = (double)(cc * sb * sa - sc * ca);  R[0][2] = (double)(cc * sb * ca + sc * sa);
    R[1][0] = (double)(sc * cb);  R[1][1] = (double)(sc * sb * sa + cc * ca);  R[1][2] = (double)(sc * sb * ca - cc * sa);
    R[2][0] = (double)-sb;        R[2][1] = (double)(cb * sa);                 R[2][2] = (double)(cb * ca);
    for (int i = 0; i < 3; i++) t[i] = x[3 + i];
}

// JJ: sum J J^T (21 values), Jr: sum J r (6 values); R and t of the update.  True when the system was solved, false: the identity.
inline bool plane_fit(const double JJ[21], const double Jr[6], double R[3][3], double t[3]) {
    double x[6], det;
    if (plane_solve6(JJ, Jr, x, &det)) {
        plane_motion(x, R, t);
        return true;
    }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = i == j ? 1.0 : 0.0;
        t[i] = 0.0;
    }
    return false;
}

}  // namespace cwipc_amd
