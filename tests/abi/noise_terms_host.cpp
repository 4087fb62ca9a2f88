// noise_terms_host.cpp -- the seeded draws, the noise filter's arithmetic and the soft camera step (csrc/counter_rng.hpp) as a
// stand-alone host program, for tests/test_noise_terms_host.py (built with -ffp-contract=off -fsanitize=address,undefined).
// noise_terms_host MODE IN OUT; a record is a run of 8-byte slots, doubles unless stated:
//   draw:  (b: uint64 | k: uint64) -> 2 slots: draw(b, k) as uint64 | u01 of it
//   noise: (u_0 .. u_3 | distance | p: 3, float32 values) -> 3 float32: the moved point on INJECTED draws
//   at:    (seed: uint64 | i: uint64 | distance | p: 3) -> 3 float32: point i of a cloud under `seed`
//   cams:  (ncam | x | z | cen_x | cen_z | skew | 0: u follows, 1: seed and index follow | u | seed: uint64 | i: uint64 | dirs: 64)
//          -> 1 int32: the camera; x, z and the centroid are float32 values, centred in float32 as the kernel does
#include "counter_rng.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned long long as_u64(double slot) {
    unsigned long long v;
    memcpy(&v, &slot, sizeof(v));
    return v;
}

int main(int argc, char **argv) {
    using namespace cwipc_amd;
    const char *modes[] = {"draw", "noise", "at", "cams"};
    const size_t widths[] = {2, 8, 6, 74};
    int mode = -1;
    for (int m = 0; argc == 4 && m < 4; m++) if (strcmp(argv[1], modes[m]) == 0) mode = m;
    if (mode < 0) {
        fprintf(stderr, "usage: noise_terms_host draw|noise|at|cams IN OUT\n");
        return 2;
    }
    const size_t nin = widths[mode];
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    std::vector<double> records;
    double rec[74];
    while (fread(rec, sizeof(double), nin, in) == nin) records.insert(records.end(), rec, rec + nin);
    fclose(in);
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    for (size_t at = 0; at + nin <= records.size(); at += nin) {
        const double *r = &records[at];
        if (mode == 0) {
            const unsigned long long x = rng_draw(as_u64(r[0]), as_u64(r[1]));
            const double u = rng_u01(x);
            if (fwrite(&x, 8, 1, out) != 1 || fwrite(&u, 8, 1, out) != 1) return 3;
        } else if (mode == 1 || mode == 2) {
            const double *pd = mode == 1 ? r + 5 : r + 3;
            const float p[3] = {(float)pd[0], (float)pd[1], (float)pd[2]};
            float res[3];
            if (mode == 1) noise_point(r, r[4], p, res);
            else noise_point_at(rng_base(as_u64(r[0]), RNG_TAG_NOISE), as_u64(r[1]), r[2], p, res);
            if (fwrite(res, sizeof(float), 3, out) != 3) return 3;
        } else {
            const int ncam = (int)r[0];
            if (ncam < 2 || ncam > 32) return 2;
            const float vx = (float)r[1] - (float)r[3], vz = (float)r[2] - (float)r[4];
            const double u = r[6] == 0.0 ? r[7] : rng_u01(rng_draw(rng_base(as_u64(r[8]), RNG_TAG_CAMS), as_u64(r[9])));
            const int cam = soft_camera(ncam, (double)vx, (double)vz, r + 10, r[5], u);
            if (fwrite(&cam, sizeof(int), 1, out) != 1) return 3;
        }
    }
    return fclose(out) == 0 ? 0 : 3;
}
