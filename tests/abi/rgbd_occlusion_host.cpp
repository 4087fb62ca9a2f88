// rgbd_occlusion_host.cpp -- the occlusion test's arithmetic (csrc/rgbd_lens.hpp: rgbd_depth_key, rgbd_colour_pixel_depth,
// rgbd_occluded, rgbd_splat_box) as a stand-alone host program, for tests/test_rgbd_occlusion_host.py (built with -ffp-contract=off
// -fsanitize=address,undefined).  All files are raw doubles unless said.
//   rgbd_occlusion_host key IN OUT       doubles (finite, > 0)                                          -> their keys, uint64
//   rgbd_occlusion_host depth IN OUT     a record is 29 doubles, as rgbd_lens_host's "colour": fxc fyc cxc cyc | the coefficients |
//                                        depth_to_colour rows 0-2 | Wc Hc | xc yc z                     -> 7 doubles: 1 / 0, uc, vc, Pz of
//                                        rgbd_colour_pixel_depth, then 1 / 0, uc, vc of rgbd_colour_pixel
//   rgbd_occlusion_host occluded IN OUT  a record is 3 doubles: Zmin Pz margin                          -> int32 1 / 0
//   rgbd_occlusion_host zbuffer IN OUT   fx fy cx cy depth_scale W H | 26 doubles, the colour side as above without the point | splat,
//                                        then W*H doubles (the depths of a sensor without depth coefficients)
//                                                                                                       -> Wc*Hc uint64: the z-buffer
//   rgbd_occlusion_host zgather IN OUT   the same input                                                 -> W*H uint64: per depth pixel Zmin at
//                                        its colour pixel as the kernels take it -- every candidate's key to its own cell, then the
//                                        minimum over the candidate's clipped square -- and the empty word for a pixel that is none
#include "rgbd_lens.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace cwipc_amd;

namespace {

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

// r: fxc fyc cxc cyc | 8 coefficients | 12 matrix entries | Wc Hc
RgbdColourTerms colour_terms(const double *r) {
    RgbdColourTerms c;
    c.fx = r[0]; c.fy = r[1]; c.cx = r[2]; c.cy = r[3];
    c.lens.k1 = r[4]; c.lens.k2 = r[5]; c.lens.p1 = r[6]; c.lens.p2 = r[7]; c.lens.k3 = r[8]; c.lens.k4 = r[9]; c.lens.k5 = r[10]; c.lens.k6 = r[11];
    for (int k = 0; k < 12; k++) c.m[k] = r[12 + k];
    c.width = (int)r[24]; c.height = (int)r[25];
    return c;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: rgbd_occlusion_host key|depth|occluded|zbuffer|zgather IN OUT\n");
        return 2;
    }
    const std::vector<double> in = read_all(argv[2]);
    if (strcmp(argv[1], "key") == 0) {
        std::vector<uint64_t> out(in.size());
        for (size_t i = 0; i < in.size(); i++) out[i] = rgbd_depth_key(in[i]);
        return write_all(argv[3], out.data(), out.size() * sizeof(uint64_t));
    }
    if (strcmp(argv[1], "depth") == 0) {
        if (in.size() % 29) return 2;
        std::vector<double> out(in.size() / 29 * 7, 0.0);
        for (size_t i = 0; i < in.size() / 29; i++) {
            const double *r = &in[29 * i];
            const RgbdColourTerms c = colour_terms(r);
            int at[2] = {0, 0};
            double pz = 0.0;
            if (rgbd_colour_pixel_depth(c, r[26], r[27], r[28], at, pz)) {
                out[7 * i] = 1.0; out[7 * i + 1] = at[0]; out[7 * i + 2] = at[1];
            }
            out[7 * i + 3] = pz;
            int old[2] = {0, 0};
            if (rgbd_colour_pixel(c, r[26], r[27], r[28], old)) {
                out[7 * i + 4] = 1.0; out[7 * i + 5] = old[0]; out[7 * i + 6] = old[1];
            }
        }
        return write_all(argv[3], out.data(), out.size() * sizeof(double));
    }
    if (strcmp(argv[1], "occluded") == 0) {
        if (in.size() % 3) return 2;
        std::vector<int32_t> out(in.size() / 3);
        for (size_t i = 0; i < out.size(); i++) out[i] = rgbd_occluded(rgbd_depth_key(in[3 * i]), in[3 * i + 1], in[3 * i + 2]) ? 1 : 0;
        return write_all(argv[3], out.data(), out.size() * sizeof(int32_t));
    }
    const bool gather = strcmp(argv[1], "zgather") == 0;
    if (gather || strcmp(argv[1], "zbuffer") == 0) {
        if (in.size() < 34) return 2;
        RgbdCamTerms t{};
        t.fx = in[0]; t.fy = in[1]; t.cx = in[2]; t.cy = in[3]; t.depth_scale = in[4];
        const int w = (int)in[5], h = (int)in[6], splat = (int)in[33];
        const RgbdColourTerms c = colour_terms(&in[7]);
        if (w < 1 || h < 1 || c.width < 1 || c.height < 1 || splat < 0 || splat > RGBD_MAX_SPLAT || in.size() != 34 + (size_t)w * h) return 2;
        std::vector<uint64_t> zbuf((size_t)c.width * c.height, RGBD_KEY_EMPTY);
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++) {
                const unsigned d = (unsigned)in[34 + (size_t)v * w + u];
                if (d == 0u) continue;
                const double z = rgbd_z(d, t.depth_scale);
                double xc, yc, pz;
                rgbd_raw_xy(t, nullptr, u, v, z, xc, yc);
                int at[2], lo[2], hi[2];
                if (!rgbd_colour_pixel_depth(c, xc, yc, z, at, pz)) continue;
                const uint64_t key = rgbd_depth_key(pz);
                rgbd_splat_box(c, at, gather ? 0 : splat, lo, hi);
                for (int r = lo[1]; r <= hi[1]; r++)
                    for (int q = lo[0]; q <= hi[0]; q++) {
                        uint64_t &cell = zbuf.at((size_t)r * c.width + q);
                        if (key < cell) cell = key;
                    }
            }
        if (!gather) return write_all(argv[3], zbuf.data(), zbuf.size() * sizeof(uint64_t));
        std::vector<uint64_t> out((size_t)w * h, RGBD_KEY_EMPTY);
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++) {
                const unsigned d = (unsigned)in[34 + (size_t)v * w + u];
                if (d == 0u) continue;
                const double z = rgbd_z(d, t.depth_scale);
                double xc, yc, pz;
                rgbd_raw_xy(t, nullptr, u, v, z, xc, yc);
                int at[2], lo[2], hi[2];
                if (!rgbd_colour_pixel_depth(c, xc, yc, z, at, pz)) continue;
                rgbd_splat_box(c, at, splat, lo, hi);
                uint64_t key_min = RGBD_KEY_EMPTY;
                for (int r = lo[1]; r <= hi[1]; r++)
                    for (int q = lo[0]; q <= hi[0]; q++) key_min = zbuf.at((size_t)r * c.width + q) < key_min ? zbuf.at((size_t)r * c.width + q) : key_min;
                out[(size_t)v * w + u] = key_min;
            }
        return write_all(argv[3], out.data(), out.size() * sizeof(uint64_t));
    }
    return 2;
}
