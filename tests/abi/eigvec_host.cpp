// eigvec_host.cpp -- the direction filter's eigen-solver (csrc/smallest_eigvec.hpp) compiled for the host, for
// tests/test_eigvec_host.py: n symmetric 3x3 matrices in (row-major, 9 doubles each), n unit vectors out.
#include "smallest_eigvec.hpp"

extern "C" void smallest_eigvec_many(const double *a, double *out, long n) {
    for (long i = 0; i < n; i++) {
        double m[3][3];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) m[r][c] = a[i * 9 + r * 3 + c];
        cwipc_amd::smallest_eigvec(m, out + i * 3);
    }
}
