// smallest_eigvec.hpp -- the direction filter's 3x3 eigen-solver, in a header of its own: kernels_direction.hip includes it for the
// device, and a host test (tests/test_eigvec_host.py, through tests/abi/eigvec_host.cpp) compiles the same text with the host
// C++ compiler and checks it against numpy.linalg.eigh.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_HOST_DEVICE __host__ __device__
#else
#define CWIPC_HOST_DEVICE
#endif

namespace cwipc_amd {

// The eigenvector of the smallest eigenvalue of a symmetric 3x3 (cyclic Jacobi in f64: rotations until the off-diagonal part is
// negligible against the whole, at most 12 sweeps; three are usually enough).  The smallest diagonal entry at the end names it,
// the lowest index on a tie.
CWIPC_HOST_DEVICE inline void smallest_eigvec(double a[3][3], double out[3]) {
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 12; sweep++) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double all = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + 2.0 * off;
        if (!(off > 1e-32 * all)) break;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; k++) {   // columns p and q
                const double akp = a[k][p], akq = a[k][q];
                a[k][p] = c * akp - s * akq;
                a[k][q] = s * akp + c * akq;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {   // rows p and q
                const double apk = a[p][k], aqk = a[q][k];
                a[p][k] = c * apk - s * aqk;
                a[q][k] = s * apk + c * aqk;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double vkp = v[k][p], vkq = v[k][q];
                v[k][p] = c * vkp - s * vkq;
                v[k][q] = s * vkp + c * vkq;
            }
        }
    }
    int m = 0;
    if (a[1][1] < a[m][m]) m = 1;
    if (a[2][2] < a[m][m]) m = 2;
    const double len = sqrt(v[0][m] * v[0][m] + v[1][m] * v[1][m] + v[2][m] * v[2][m]);
    for (int k = 0; k < 3; k++) out[k] = v[k][m] / len;
}

}  // namespace cwipc_amd
