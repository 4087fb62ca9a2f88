// quality_terms_host.cpp -- RULE Q's per-pair arithmetic (csrc/quality_terms.hpp) as a stand-alone host program, for
// tests/test_quality_terms_host.py (built with -ffp-contract=off -fsanitize=address,undefined).  quality_terms_host IN OUT:
//   records of 13 doubles (p: 3 | q: 3 | m: 3 | 1: the pair has a normal, 0: it has none | the source's packed colour word | the
//   reference's | d2) -> 10 doubles, the terms
#include "quality_terms.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: quality_terms_host IN OUT\n");
        return 2;
    }
    const size_t nin = 13, nout = cwipc_amd::QUALITY_NTERM;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<double> records;
    double rec[13];
    while (fread(rec, sizeof(double), nin, in) == nin) records.insert(records.end(), rec, rec + nin);
    fclose(in);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (size_t i = 0; i + nin <= records.size(); i += nin) {
        const double *r = &records[i];
        double res[cwipc_amd::QUALITY_NTERM];
        cwipc_amd::quality_pair_terms(r, r + 3, r + 6, r[9] != 0.0,(uint32_t)r[10], (uint32_t)r[11], r[12], res);
        if (fwrite(res, sizeof(double), nout, out) != nout) return 3;
    }
    return fclose(out) == 0 ? 0 : 3;
}
