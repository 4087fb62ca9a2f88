// rgbd_depthfilter_host.cpp -- the depth post-processing's arithmetic (csrc/rgbd_depthfilter.hpp: rgbd_line_step through rgbd_line_pass,
// rgbd_temporal_step, rgbd_persists) as a stand-alone host program, for tests/test_rgbd_depthfilter_host.py (built with
// -ffp-contract=off -fsanitize=address,undefined).  All files are raw doubles unless said.
//   rgbd_depthfilter_host lines IN OUT     alpha delta backward(0 / 1), then per line: n, then n depths   -> the lines after one pass, uint16,
//                                          one after the other
//   rgbd_depthfilter_host spatial IN OUT   alpha delta magnitude W H, then W*H depths                     -> W*H uint16: rule 0a
//   rgbd_depthfilter_host temporal IN OUT  alpha delta, then records of 4 doubles: mode c s h             -> per record 3 doubles: out s h
//   rgbd_depthfilter_host persists IN OUT  (nothing read)                                                 -> 9 * 256 bytes, 1 / 0
#include "rgbd_depthfilter.hpp"

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

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: rgbd_depthfilter_host lines|spatial|temporal|persists IN OUT\n");
        return 2;
    }
    const std::vector<double> in = read_all(argv[2]);
    if (strcmp(argv[1], "persists") == 0) {
        std::vector<uint8_t> out;
        for (int mode = 0; mode <= RGBD_MAX_PERSISTENCY; mode++)
            for (unsigned h = 0; h < 256u; h++) out.push_back(rgbd_persists(mode, h) ? 1 : 0);
        return write_all(argv[3], out.data(), out.size());
    }
    if (in.size() < 2) return 2;
    const RgbdSmoothTerms t = rgbd_smooth_terms(in[0], in[1]);
    if (strcmp(argv[1], "lines") == 0) {
        if (in.size() < 3) return 2;
        const bool backward = in[2] != 0.0;
        std::vector<uint16_t> out;
        size_t at = 3;
        while (at < in.size()) {
            const size_t n = (size_t)in[at++];
            if (n < 1 || at + n > in.size()) return 2;
            std::vector<uint16_t> line(n);   // (a vector of its own per line: the sanitizer sees a step outside it)
            for (size_t i = 0; i < n; i++) line[i] = (uint16_t)in[at + i];
            rgbd_line_pass(t, line.data(), n, 1, backward);
            out.insert(out.end(), line.begin(), line.end());
            at += n;
        }
        return write_all(argv[3], out.data(), out.size() * sizeof(uint16_t));
    }
    if (strcmp(argv[1], "spatial") == 0) {
        if (in.size() < 5) return 2;
        const int magnitude = (int)in[2];
        const size_t w = (size_t)in[3], h = (size_t)in[4];
        if (magnitude < 0 || magnitude > RGBD_MAX_SPATIAL_MAGNITUDE || w < 1 || h < 1 || in.size() != 5 + w * h) return 2;
        std::vector<uint16_t> image(w * h);
        for (size_t i = 0; i < w * h; i++) image[i] = (uint16_t)in[5 + i];
        for (int it = 0; it < magnitude; it++) {
            for (size_t v = 0; v < h; v++) rgbd_line_pass(t, &image[v * w], w, 1, false);
            for (size_t v = 0; v < h; v++) rgbd_line_pass(t, &image[v * w], w, 1, true);
            for (size_t u = 0; u < w; u++) rgbd_line_pass(t, &image[u], h, w, false);
            for (size_t u = 0; u < w; u++) rgbd_line_pass(t, &image[u], h, w, true);
        }
        return write_all(argv[3], image.data(), image.size() * sizeof(uint16_t));
    }
    if (strcmp(argv[1], "temporal") == 0) {
        if ((in.size() - 2) % 4) return 2;
        const size_t n = (in.size() - 2) / 4;
        std::vector<double> out(3 * n);
        for (size_t i = 0; i < n; i++) {
            const double *r = &in[2 + 4 * i];
            double s = r[2];
            uint8_t h = (uint8_t)r[3];
            out[3 * i] = (double)rgbd_temporal_step(t, (int)r[0], (uint16_t)r[1], s, h);
            out[3 * i + 1] = s;
            out[3 * i + 2] = (double)h;
        }
        return write_all(argv[3], out.data(), out.size() * sizeof(double));
    }
    return 2;
}
