// gicp_terms.hpp -- the arithmetic of generalized ICP that is new against point-to-plane (kernels_icp.hip): the orientation of a
// normal, the covariance of a point from its normal, the terms of a matched pair.  No HIP type: the kernels include it, and a host
// test (tests/test_gicp_terms_host.py, through tests/abi/gicp_terms_host.cpp) compiles the same text with the host C++ compiler and
// checks it bit for bit against the numpy model (tests/icp_gicp_model.py).  Every operation is rounded on its own, in f64
// (-ffp-contract=off); the order of the operations below IS the contract.
//
// A restatement of open3d's registration_generalized_icp (TransformationEstimationForGeneralizedICP, L2 loss) -- open3d is not on this
// stack.  open3d writes W = (M^-1)^(1/2), J = W A, r = W e; W is symmetric, so J^T J = A^T N A, J^T r = A^T g and r^T r = e^T g with
// N = M^-1 and g = N e: no matrix square root, no eigen-solve.  M = Ct + R Cs R^T has eigenvalues between 2 eps and about 2, so
// the inverse by cofactors is well conditioned.
#pragma once

#include <cmath>

#ifndef CWIPC_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_HOST_DEVICE __host__ __device__
#else
#define CWIPC_HOST_DEVICE
#endif
#endif

namespace cwipc_amd {

constexpr int GICP_NTERM = 30;   // 1 | (A^T N A)_ij for i <= j (21) | (A^T g)_i (6) | e^T g | d2

// open3d's OrientNormalsToAlignWithDirection: a zero normal becomes the direction d, a normal that points against d is negated.
// A comparison with NaN is false: a NaN direction never flips a normal.
CWIPC_HOST_DEVICE inline void gicp_orient(double m[3], const double d[3]) {
    if (m[0] == 0.0 && m[1] == 0.0 && m[2] == 0.0) {
        m[0] = d[0]; m[1] = d[1]; m[2] = d[2];
    } else if ((m[0] * d[0] + m[1] * d[1]) + m[2] * d[2] < 0.0) {
        m[0] = -m[0]; m[1] = -m[1]; m[2] = -m[2];
    }
}

// open3d's GetRotationFromE1ToX(m) followed by C = Rx diag(eps, 1, 1) Rx^T; C as 00, 01, 02, 11, 12, 22.  Rx = I for m0 < -0.99:
// open3d's rule as published, the covariance is then diag(eps, 1, 1) for every normal within about 8 degrees of -x.
CWIPC_HOST_DEVICE inline void gicp_covariance(const double m[3], double eps, double C[6]) {
    double Rx[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    const double c = m[0];
    if (!(c < -0.99)) {
        const double f = 1.0 / (1.0 + c);
        Rx[0][0] = 1.0 - f * (m[1] * m[1] + m[2] * m[2]);
        Rx[0][1] = -m[1];
        Rx[0][2] = -m[2];
        Rx[1][0] = m[1];
        Rx[1][1] = 1.0 - f * (m[1] * m[1]);
        Rx[1][2] = -(f * (m[1] * m[2]));
        Rx[2][0] = m[2];
        Rx[2][1] = -(f * (m[1] * m[2]));
        Rx[2][2] = 1.0 - f * (m[2] * m[2]);
    }
    int v = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) C[v++] = ((eps * Rx[i][0]) * Rx[j][0] + Rx[i][1] * Rx[j][1]) + Rx[i][2] * Rx[j][2];
}

// The 30 terms of a matched pair: p the moved source point, q the matched reference point, Cs and Ct their covariances (six values
// each, as gicp_covariance writes them), R the 3x3 block of T (row-major), d2 the pair's squared distance.
CWIPC_HOST_DEVICE inline void gicp_pair_terms(const double p[3], const double q[3], const double Cs[6], const double Ct[6], const double R[9], double d2,
                                              double out[GICP_NTERM]) {
    const double cs[3][3] = {{Cs[0], Cs[1], Cs[2]}, {Cs[1], Cs[3], Cs[4]}, {Cs[2], Cs[4], Cs[5]}};
    // B = R Cs, S = B R^T (its upper triangle), M = Ct + S
    double B[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) B[i][j] = (R[3 * i] * cs[0][j] + R[3 * i + 1] * cs[1][j]) + R[3 * i + 2] * cs[2][j];
    double M[6];
#pragma unroll
    for (int i = 0, v = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++, v++) M[v] = Ct[v] + ((B[i][0] * R[3 * j] + B[i][1] * R[3 * j + 1]) + B[i][2] * R[3 * j + 2]);
    const double M00 = M[0], M01 = M[1], M02 = M[2], M11 = M[3], M12 = M[4], M22 = M[5];
    // N = M^-1 by cofactors
    const double k00 = M11 * M22 - M12 * M12, k01 = M02 * M12 - M01 * M22, k02 = M01 * M12 - M02 * M11;
    const double k11 = M00 * M22 - M02 * M02, k12 = M01 * M02 - M00 * M12, k22 = M00 * M11 - M01 * M01;
    const double det = (M00 * k00 + M01 * k01) + M02 * k02;
    const double n00 = k00 / det, n01 = k01 / det, n02 = k02 / det, n11 = k11 / det, n12 = k12 / det, n22 = k22 / det;
    const double N[3][3] = {{n00, n01, n02}, {n01, n11, n12}, {n02, n12, n22}};
    const double e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    double g[3];
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] = (N[i][0] * e[0] + N[i][1] * e[1]) + N[i][2] * e[2];
    // A = [-skew(p) | I]; H = N A; then A^T H, A^T g, e^T g
    const double A[3][6] = {{0.0, p[2], -p[1], 1.0, 0.0, 0.0}, {-p[2], 0.0, p[0], 0.0, 1.0, 0.0}, {p[1], -p[0], 0.0, 0.0, 0.0, 1.0}};
    double H[3][6];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) H[i][j] = (N[i][0] * A[0][j] + N[i][1] * A[1][j]) + N[i][2] * A[2][j];
    int v = 0;
    out[v++] = 1.0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) out[v++] = (A[0][i] * H[0][j] + A[1][i] * H[1][j]) + A[2][i] * H[2][j];
#pragma unroll
    for (int i = 0; i < 6; i++) out[v++] = (A[0][i] * g[0] + A[1][i] * g[1]) + A[2][i] * g[2];
    out[v++] = (e[0] * g[0] + e[1] * g[1]) + e[2] * g[2];
    out[v++] = d2;
}

}  // namespace cwipc_amd
