// rgbd_decimate_host.cpp -- the decimation and hole-filling arithmetic (csrc/rgbd_decimate.hpp: rgbd_derived_grid, rgbd_block_value
// through rgbd_decimate_image, rgbd_fill_op and rgbd_fill_pick through rgbd_holefill_image) as a stand-alone host program, for
// tests/test_rgbd_decimate_host.py (built with -ffp-contract=off -fsanitize=address,undefined).  All files are raw doubles unless said.
//   rgbd_decimate_host decimate IN OUT   records: k W H, then W*H depths      -> per record (W div k)*(H div k) uint16, one after the other
//   rgbd_decimate_host sensor IN OUT     records of 7: k W H fx fy cx cy      -> per record 6 doubles: W' H' fx' fy' cx' cy'
//   rgbd_decimate_host fill IN OUT       records: mode W H, then W*H depths   -> per record W*H uint16: rule 0c
#include "rgbd_decimate.hpp"

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
        fprintf(stderr, "usage: rgbd_decimate_host decimate|sensor|fill IN OUT\n");
        return 2;
    }
    const std::vector<double> in = read_all(argv[2]);
    if (strcmp(argv[1], "sensor") == 0) {
        if (in.size() % 7) return 2;
        std::vector<double> out;
        for (size_t at = 0; at < in.size(); at += 7) {
            const int k = (int)in[at];
            if (k < 1 || k > RGBD_MAX_DECIMATION) return 2;
            const RgbdGrid g = rgbd_derived_grid((int)in[at + 1], (int)in[at + 2], in[at + 3], in[at + 4], in[at + 5], in[at + 6], k);
            const double record[6] = {(double)g.width, (double)g.height, g.fx, g.fy, g.cx, g.cy};
            out.insert(out.end(), record, record + 6);
        }
        return write_all(argv[3], out.data(), out.size() * sizeof(double));
    }
    const bool fill = strcmp(argv[1], "fill") == 0;
    if (!fill && strcmp(argv[1], "decimate") != 0) return 2;
    std::vector<uint16_t> out;
    size_t at = 0;
    while (at < in.size()) {
        if (at + 3 > in.size()) return 2;
        const int arg = (int)in[at];
        const size_t w = (size_t)in[at + 1], h = (size_t)in[at + 2];
        at += 3;
        if (w < 1 || h < 1 || at + w * h > in.size()) return 2;
        std::vector<uint16_t> image(w * h);   // (vectors of their own per image: the sanitizer sees a step outside one)
        for (size_t i = 0; i < w * h; i++) image[i] = (uint16_t)in[at + i];
        at += w * h;
        if (fill) {
            if (arg < 1 || arg > RGBD_MAX_HOLEFILL) return 2;
            std::vector<uint16_t> result(w * h);
            rgbd_holefill_image(arg, image.data(), w, h, result.data());
            out.insert(out.end(), result.begin(), result.end());
        } else {
            if (arg < 2 || arg > RGBD_MAX_DECIMATION) return 2;   // (an image lower or narrower than k decimates to nothing)
            std::vector<uint16_t> result((w / (size_t)arg) * (h / (size_t)arg));
            if (!rgbd_decimate_image(image.data(), w, h, arg, result.data())) return 2;
            out.insert(out.end(), result.begin(), result.end());
        }
    }
    return write_all(argv[3], out.data(), out.size() * sizeof(uint16_t));
}
