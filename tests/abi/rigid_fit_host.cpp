// rigid_fit_host.cpp -- the ICP step's rigid fit (csrc/rigid_fit.hpp) as a stand-alone host program, for
// tests/test_rigid_fit_host.py (built with -fsanitize=address,undefined).  Reads a file of records of 22 doubles
// (n | sum a (3) | sum b (3) | sum a b^T (9) | cp (3) | cq (3)), writes 12 doubles per record (R row-major, t).
#include "rigid_fit.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: rigid_fit_host IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<double> records;
    double rec[22];
    while (fread(rec, sizeof(double), 22, in) == 22) records.insert(records.end(), rec, rec + 22);
    fclose(in);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (size_t i = 0; i + 22 <= records.size(); i += 22) {
        const double *r = &records[i];
        double R[3][3], t[3], flat[12];
        cwipc_amd::rigid_fit((uint64_t)r[0], r + 1, r + 4, r + 7, r + 16, r + 19, R, t);
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) flat[3 * a + b] = R[a][b];
            flat[9 + a] = t[a];
        }
        if (fwrite(flat, sizeof(double), 12, out) != 12) return 3;
    }
    return fclose(out) == 0 ? 0 : 3;
}
