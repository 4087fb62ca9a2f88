// rgbd_lens_host.cpp -- the arithmetic of the RGB-D source's raw entry (csrc/rgbd_lens.hpp) as a stand-alone host program, for
// tests/test_rgbd_lens_host.py (built with -ffp-contract=off -fsanitize=address,undefined).  All files are raw doubles unless said.
//   rgbd_lens_host distort IN OUT   a record is 10 doubles: k1 k2 p1 p2 k3 k4 k5 k6 | x y              -> 2 doubles: x' y'
//   rgbd_lens_host table IN OUT     one record of 14 doubles: the coefficients | fx fy cx cy | W H     -> 2*W*H doubles, the ray table
//   rgbd_lens_host colour IN OUT    a record is 29 doubles: fxc fyc cxc cyc | the coefficients | depth_to_colour rows 0-2: 12 | Wc Hc |
//                                   xc yc z                                                            -> 3 int32: 1 / 0, uc, vc
//   rgbd_lens_host erode IN OUT     4 doubles W H ex ey, then W*H doubles (the depths)                 -> W*H doubles: the eroded depths,
//                                   through rgbd_erode_word on 64-pixel words as the kernels do it
#include "rgbd_lens.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace cwipc_amd;

namespace {

RgbdLens lens_of(const double *k) {
    RgbdLens l;
    l.k1 = k[0]; l.k2 = k[1]; l.p1 = k[2]; l.p2 = k[3]; l.k3 = k[4]; l.k4 = k[5]; l.k5 = k[6]; l.k6 = k[7];
    return l;
}

std::vector<double> read_all(const char *path) {
    std::vector<double> rv;
    FILE *in = fopen(path, "rb");
    if (!in) return rv;
    double buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(double), 4096, in)) > 0) rv.insert(rv.end(), buf, buf + n);
    fclose(in);
    return rv;
}

int write_all(const char *path, const void *data, size_t bytes) {
    FILE *out = fopen(path, "wb");
    if (!out) return 3;
    if (bytes && fwrite(data, 1, bytes, out) != bytes) return 3;
    return fclose(out) == 0 ? 0 : 3;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: rgbd_lens_host distort|table|colour|erode IN OUT\n");
        return 2;
    }
    const std::vector<double> in = read_all(argv[2]);
    if (strcmp(argv[1], "distort") == 0) {
        if (in.size() % 10) return 2;
        std::vector<double> out(in.size() / 10 * 2);
        for (size_t i = 0; i < in.size() / 10; i++) rgbd_distort(lens_of(&in[10 * i]), in[10 * i + 8], in[10 * i + 9], &out[2 * i]);
        return write_all(argv[3], out.data(), out.size() * sizeof(double));
    }
    if (strcmp(argv[1], "table") == 0) {
        if (in.size() != 14) return 2;
        const RgbdLens l = lens_of(&in[0]);
        RgbdCamTerms c{};
        c.fx = in[8]; c.fy = in[9]; c.cx = in[10]; c.cy = in[11];
        const int w = (int)in[12], h = (int)in[13];
        std::vector<double> out((size_t)w * h * 2);
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++) rgbd_ray(c, l, u, v, &out[2 * ((size_t)v * w + u)]);
        return write_all(argv[3], out.data(), out.size() * sizeof(double));
    }
    if (strcmp(argv[1], "colour") == 0) {
        if (in.size() % 29) return 2;
        std::vector<int32_t> out(in.size() / 29 * 3, 0);
        for (size_t i = 0; i < in.size() / 29; i++) {
            const double *r = &in[29 * i];
            RgbdColourTerms c;
            c.fx = r[0]; c.fy = r[1]; c.cx = r[2]; c.cy = r[3];
            c.lens = lens_of(r + 4);
            for (int k = 0; k < 12; k++) c.m[k] = r[12 + k];
            c.width = (int)r[24]; c.height = (int)r[25];
            int at[2] = {0, 0};
            if (rgbd_colour_pixel(c, r[26], r[27], r[28], at)) {
                out[3 * i] = 1; out[3 * i + 1] = at[0]; out[3 * i + 2] = at[1];
            }
        }
        return write_all(argv[3], out.data(), out.size() * sizeof(int32_t));
    }
    if (strcmp(argv[1], "erode") == 0) {
        if (in.size() < 4) return 2;
        const int w = (int)in[0], h = (int)in[1], ex = (int)in[2], ey = (int)in[3];
        if (w < 1 || h < 1 || in.size() != 4 + (size_t)w * h || ex < 0 || ex > RGBD_MAX_EROSION || ey < 0 || ey > RGBD_MAX_EROSION) return 2;
        const double *d = &in[4];
        const int wpr = (w + 63) / 64;
        std::vector<unsigned long long> valid((size_t)h * wpr), rows((size_t)h * wpr);
        for (int v = 0; v < h; v++)
            for (int i = 0; i < wpr; i++) {
                unsigned long long word = 0;
                for (int b = 0; b < 64; b++) {
                    const int u = 64 * i + b;
                    if (u >= w || d[(size_t)v * w + u] != 0.0) word |= 1ull << b;
                }
                valid[(size_t)v * wpr + i] = word;
            }
        for (int v = 0; v < h; v++)
            for (int i = 0; i < wpr; i++) {
                const unsigned long long *row = &valid[(size_t)v * wpr];
                rows[(size_t)v * wpr + i] = rgbd_erode_word(i > 0 ? row[i - 1] : ~0ull, row[i], i + 1 < wpr ? row[i + 1] : ~0ull, ex);
            }
        std::vector<double> out((size_t)w * h);
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++) {
                unsigned long long word = ~0ull;
                for (int dv = -ey; dv <= ey; dv++)
                    if (v + dv >= 0 && v + dv < h) word &= rows[(size_t)(v + dv) * wpr + u / 64];
                out[(size_t)v * w + u] = ((word >> (u & 63)) & 1ull) ? d[(size_t)v * w + u] : 0.0;
            }
        return write_all(argv[3], out.data(), out.size() * sizeof(double));
    }
    return 2;
}
