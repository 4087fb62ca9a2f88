// plane_seg_host.cpp -- the arithmetic of plane segmentation (csrc/plane_seg_terms.hpp with csrc/counter_rng.hpp and
// csrc/smallest_eigvec.hpp) as a stand-alone host program, for tests/test_plane_seg_host.py, which builds it with
// -fsanitize=address,undefined and runs it as a program.
//   plane_seg_host find IN OUT distance H seed ax ay az min_abs_cos flags
//        IN: n cwipc_point records (16 bytes each).  OUT: the result in the layout of cwipc_hip_plane_result (232 bytes), then the
//        table: 4 H doubles, H uint32 counts, H validity bytes (the header's plane_find_brute)
//   plane_seg_host refit distance ax ay az min_abs_cos count recount a0 a1 a2 h0 h1 h2 h3 s0 .. s9
//        the decision after best and sums: prints wanted, refined, then plane[4] and M[6] as hexadecimal doubles
//   plane_seg_host offsets distance a0 a1 a2 p0 p1 p2       prints takes-part (0 / 1) and the three quantised offsets
//   plane_seg_host level n0 n1 n2 d                          prints ok (0 / 1) and the 16 entries as hexadecimal doubles
//   plane_seg_host rule distance H min_abs_cos               prints plane_rule_ok (0 / 1) with a zero axis
#include "plane_seg_terms.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

using namespace cwipc_amd;

struct Point {
    float x, y, z;
    uint8_t r, g, b, tile;
};
static_assert(sizeof(Point) == 16, "a cwipc_point is 16 bytes");

struct Result {   // cwipc_hip_plane_result
    double plane[4], hypothesis[4];
    int64_t sums[10];
    double M[6];
    uint32_t best, triple[3], count, recount, valid;
    int32_t found, refined, reserved;
};
static_assert(sizeof(Result) == 232, "the layout of cwipc_hip_plane_result");

Result result_of(const PlaneFound &f) {
    Result r;
    memset(&r, 0, sizeof(r));
    for (int a = 0; a < 4; a++) { r.plane[a] = f.plane[a]; r.hypothesis[a] = f.hypothesis[a]; }
    for (int i = 0; i < 10; i++) r.sums[i] = (int64_t)f.sums[i];
    for (int i = 0; i < 6; i++) r.M[i] = f.M[i];
    r.best = f.best;
    for (int k = 0; k < 3; k++) r.triple[k] = f.triple[k];
    r.count = f.count; r.recount = f.recount; r.valid = f.valid; r.found = f.found; r.refined = f.refined;
    return r;
}

int find(int argc, char **argv) {
    if (argc != 12) return 2;
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 3;
    std::vector<Point> pts;
    Point p;
    while (fread(&p, sizeof(p), 1, in) == 1) pts.push_back(p);
    fclose(in);
    const double distance = strtod(argv[4], nullptr);
    const uint32_t H = (uint32_t)strtoul(argv[5], nullptr, 10);
    const unsigned long long seed = strtoull(argv[6], nullptr, 10);
    const double axis[3] = {strtod(argv[7], nullptr), strtod(argv[8], nullptr), strtod(argv[9], nullptr)};
    const double mac = strtod(argv[10], nullptr);
    const int flags = atoi(argv[11]);
    if (!plane_rule_ok(distance, H, axis, mac)) return 4;
    const PlaneRule r = plane_rule(distance, H, seed, axis, mac);
    std::vector<double> planes(4 * (size_t)H);
    std::vector<uint32_t> counts(H);
    std::vector<uint8_t> valid(H);
    PlaneFound f;
    plane_find_brute(pts.data(), pts.size(), r, (flags & 1) != 0, f, planes.data(), counts.data(), valid.data());
    const Result res = result_of(f);
    FILE *of = fopen(argv[3], "wb");
    if (!of) return 3;
    bool ok = fwrite(&res, sizeof(res), 1, of) == 1;
    ok = ok && fwrite(planes.data(), sizeof(double), planes.size(), of) == planes.size();
    ok = ok && fwrite(counts.data(), sizeof(uint32_t), counts.size(), of) == counts.size();
    ok = ok && fwrite(valid.data(), 1, valid.size(), of) == valid.size();
    fclose(of);
    return ok ? 0 : 3;
}

int refit(int argc, char **argv) {
    if (argc != 26) return 2;
    const double distance = strtod(argv[2], nullptr);
    const double axis[3] = {strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtod(argv[5], nullptr)};
    const PlaneRule r = plane_rule(distance, 1, 0, axis, strtod(argv[6], nullptr));
    PlaneFound f;
    f.found = 1;
    f.count = (uint32_t)strtoul(argv[7], nullptr, 10);
    const uint32_t recount = (uint32_t)strtoul(argv[8], nullptr, 10);
    const double anchor[3] = {strtod(argv[9], nullptr), strtod(argv[10], nullptr), strtod(argv[11], nullptr)};
    for (int a = 0; a < 4; a++) f.hypothesis[a] = strtod(argv[12 + a], nullptr);
    for (int i = 0; i < 10; i++) f.sums[i] = (uint64_t)strtoll(argv[16 + i], nullptr, 10);
    double plane[4] = {0, 0, 0, 0};
    const bool wanted = plane_refit_wanted(r, f, anchor, plane);
    plane_conclude(r, f, wanted, plane, recount);
    printf("%d\n%d\n", wanted ? 1 : 0, f.refined);
    for (int a = 0; a < 4; a++) printf("%a\n", f.plane[a]);
    for (int i = 0; i < 6; i++) printf("%a\n", f.M[i]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "find")) return find(argc, argv);
    if (!strcmp(argv[1], "refit")) return refit(argc, argv);
    if (!strcmp(argv[1], "offsets") && argc == 9) {
        const double distance = strtod(argv[2], nullptr);
        const double anchor[3] = {strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtod(argv[5], nullptr)};
        const double p[3] = {strtod(argv[6], nullptr), strtod(argv[7], nullptr), strtod(argv[8], nullptr)};
        int64_t o[3];
        const bool ok = plane_offsets(p, anchor, PLANE_FIX / distance, o);
        printf("%d\n%lld\n%lld\n%lld\n", ok ? 1 : 0, (long long)o[0], (long long)o[1], (long long)o[2]);
        return 0;
    }
    if (!strcmp(argv[1], "level") && argc == 6) {
        const double plane[4] = {strtod(argv[2], nullptr), strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtod(argv[5], nullptr)};
        double m[16];
        memset(m, 0, sizeof(m));
        printf("%d\n", plane_level_matrix(plane, m) ? 1 : 0);
        for (int i = 0; i < 16; i++) printf("%a\n", m[i]);
        return 0;
    }
    if (!strcmp(argv[1], "rule") && argc == 5) {
        const double axis[3] = {0, 0, 0};
        printf("%d\n", plane_rule_ok(strtod(argv[2], nullptr), (uint32_t)strtoul(argv[3], nullptr, 10), axis, strtod(argv[4], nullptr)) ? 1 : 0);
        return 0;
    }
    return 2;
}
