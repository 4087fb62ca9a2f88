// gicp_terms_host.cpp -- generalized ICP's per-point and per-pair arithmetic (csrc/gicp_terms.hpp) as a stand-alone host program, for
// tests/test_gicp_terms_host.py (built with -ffp-contract=off -fsanitize=address,undefined).  gicp_terms_host MODE IN OUT:
//   cov:  records of 8 doubles (normal: 3 | direction: 3 | 1: orient first, 0: do not | epsilon) -> 6 doubles, the covariance
//   pair: records of 28 doubles (p: 3 | q: 3 | Cs: 6 | Ct: 6 | R row-major: 9 | d2) -> 30 doubles, the terms
#include "gicp_terms.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 4 || (strcmp(argv[1], "cov") != 0 && strcmp(argv[1], "pair") != 0)) {
        fprintf(stderr, "usage: gicp_terms_host cov|pair IN OUT\n");
        return 2;
    }
    const bool cov = strcmp(argv[1], "cov") == 0;
    const size_t nin = cov ? 8 : 28, nout = cov ? 6 : cwipc_amd::GICP_NTERM;
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    std::vector<double> records;
    double rec[28];
    while (fread(rec, sizeof(double), nin, in) == nin) records.insert(records.end(), rec, rec + nin);
    fclose(in);
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    for (size_t i = 0; i + nin <= records.size(); i += nin) {
        const double *r = &records[i];
        double res[cwipc_amd::GICP_NTERM];
        if (cov) {
            double m[3] = {r[0], r[1], r[2]};
            if (r[6] != 0.0) cwipc_amd::gicp_orient(m, r + 3);
            cwipc_amd::gicp_covariance(m, r[7], res);
        } else {
            cwipc_amd::gicp_pair_terms(r, r + 3, r + 6, r + 12, r + 18, r[27], res);
        }
        if (fwrite(res, sizeof(double), nout, out) != nout) return 3;
    }
    return fclose(out) == 0 ? 0 : 3;
}
