// plane_fit_host.cpp -- the point-to-plane ICP step's 6x6 solve and motion (csrc/plane_fit.hpp) as a stand-alone host program, for
// tests/test_plane_fit_host.py (built with -fsanitize=address,undefined).  Reads a file of records of 27 doubles
// (sum J J^T: 21, upper triangle row-major | sum J r: 6), writes 20 doubles per record:
// x (6; zeros when not solved) | det | solved (1 or 0) | R row-major (9) | t (3).
#include "plane_fit.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: plane_fit_host IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<double> records;
    double rec[27];
    while (fread(rec, sizeof(double), 27, in) == 27) records.insert(records.end(), rec, rec + 27);
    fclose(in);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (size_t i = 0; i + 27 <= records.size(); i += 27) {
        const double *r = &records[i];
        double flat[20] = {0}, R[3][3], t[3];
        flat[7] = cwipc_amd::plane_solve6(r, r + 21, flat, &flat[6]) ? 1.0 : 0.0;
        const bool fitted = cwipc_amd::plane_fit(r, r + 21, R, t);
        if (fitted != (flat[7] == 1.0)) return 4;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) flat[8 + 3 * a + b] = R[a][b];
            flat[17 + a] = t[a];
        }
        if (fwrite(flat, sizeof(double), 20, out) != 20) return 3;
    }
    return fclose(out) == 0 ? 0 : 3;
}
