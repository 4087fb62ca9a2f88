// smooth_host.cpp -- the smoothing's per-point arithmetic (csrc/smooth_terms.hpp with csrc/smallest_eigvec.hpp) as a stand-alone
// host program, for tests/test_smooth_host.py, which builds it with -fsanitize=address,undefined and runs it as a program.
//   smooth_host smooth IN OUT radius flags min_neighbours   IN: n cwipc_point records (16 bytes each); OUT: the same, smoothed by
//                                                           brute force over all pairs (the header's smooth_brute_force)
//   smooth_host moves min_neighbours cnt...                 prints smooth_moves(cnt, min_neighbours) for every cnt, 0 or 1
//   smooth_host radius r...                                 prints smooth_radius_ok(r) for every r, 0 or 1
#include "smooth_terms.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Point {
    float x, y, z;
    uint8_t r, g, b, tile;
};
static_assert(sizeof(Point) == 16, "a cwipc_point is 16 bytes");

int smooth(int argc, char **argv) {
    if (argc != 7) return 2;
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 3;
    std::vector<Point> pts;
    Point p;
    while (fread(&p, sizeof(p), 1, in) == 1) pts.push_back(p);
    fclose(in);
    const double radius = strtod(argv[4], nullptr);
    const int flags = atoi(argv[5]);
    const uint32_t min_neighbours = (uint32_t)strtoul(argv[6], nullptr, 10);
    if (!cwipc_amd::smooth_radius_ok(radius)) return 4;
    std::vector<Point> out(pts.size());
    cwipc_amd::smooth_brute_force(pts.data(), pts.size(), radius, (flags & 1) != 0, min_neighbours, out.data());
    FILE *of = fopen(argv[3], "wb");
    if (!of) return 3;
    const bool ok = out.empty() || fwrite(out.data(), sizeof(Point), out.size(), of) == out.size();
    fclose(of);
    return ok ? 0 : 3;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "smooth")) return smooth(argc, argv);
    if (!strcmp(argv[1], "moves") && argc >= 3) {
        const uint32_t min_neighbours = (uint32_t)strtoul(argv[2], nullptr, 10);
        for (int k = 3; k < argc; k++) printf("%d\n", cwipc_amd::smooth_moves(strtoull(argv[k], nullptr, 10), min_neighbours) ? 1 : 0);
        return 0;
    }
    if (!strcmp(argv[1], "radius")) {
        for (int k = 2; k < argc; k++) printf("%d\n", cwipc_amd::smooth_radius_ok(strtod(argv[k], nullptr)) ? 1 : 0);
        return 0;
    }
    return 2;
}
