// rgbd_terms_host.cpp -- the RGB-D source's per-pixel arithmetic (csrc/rgbd_terms.hpp) as a stand-alone host program, for
// tests/test_rgbd_terms_host.py (built with -ffp-contract=off -fsanitize=address,undefined).
//   rgbd_terms_host pixel IN OUT   a record is 29 doubles: fx fy cx cy depth_scale | m: 12 | near far height_min height_max radius green |
//                                  u v d | r g b   ->  4 32-bit words: 1 kept / 0 dropped | the point's x, y, z as float32 (computed
//                                  whenever d != 0, kept or not; zeros for d = 0)
//   rgbd_terms_host green OUT      2^24 bits, bit (r | g << 8 | b << 16) set iff rgbd_not_green(r, g, b)
#include "rgbd_terms.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
    using namespace cwipc_amd;
    if (argc == 3 && strcmp(argv[1], "green") == 0) {
        std::vector<uint8_t> mask((size_t)1 << 21, 0);
        for (unsigned c = 0; c < (1u << 24); c++)
            if (rgbd_not_green(c & 255u, (c >> 8) & 255u, (c >> 16) & 255u)) mask[c >> 3] |= (uint8_t)(1u << (c & 7u));
        FILE *out = fopen(argv[2], "wb");
        if (!out || fwrite(mask.data(), 1, mask.size(), out) != mask.size()) return 3;
        return fclose(out) == 0 ? 0 : 3;
    }
    if (argc != 4 || strcmp(argv[1], "pixel") != 0) {
        fprintf(stderr, "usage: rgbd_terms_host pixel IN OUT | green OUT\n");
        return 2;
    }
    constexpr size_t NIN = 29;
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    double r[NIN];
    while (fread(r, sizeof(double), NIN, in) == NIN) {
        RgbdCamTerms c;
        c.fx = r[0]; c.fy = r[1]; c.cx = r[2]; c.cy = r[3]; c.depth_scale = r[4];
        for (int i = 0; i < 12; i++) c.m[i] = r[5 + i];
        RgbdFilterTerms f;
        f.near_z = r[17]; f.far_z = r[18]; f.height_min = r[19]; f.height_max = r[20]; f.radius = (float)r[21]; f.green = (int)r[22];
        const int u = (int)r[23], v = (int)r[24];
        const unsigned d = (unsigned)r[25];
        const unsigned colour = (unsigned)r[26] | ((unsigned)r[27] << 8) | ((unsigned)r[28] << 16);
        uint32_t res[4] = {0, 0, 0, 0};
        res[0] = rgbd_keep(c, f, rgbd_active(f), u, v, d, [=]() { return colour; }) ? 1u : 0u;
        if (d != 0u) {
            float pt[3];
            rgbd_point(c, u, v, d, pt);
            memcpy(res + 1, pt, sizeof(pt));
        }
        if (fwrite(res, sizeof(uint32_t), 4, out) != 4) return 3;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
