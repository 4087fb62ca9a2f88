// The octree codec's arithmetic and packet validator (csrc/codec_terms.hpp) compiled for the host, stand-alone, for
// tests/test_codec_packet_host.py: built with -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all.
//   codec_packet_host cells IN OUT      IN: doubles bits, n, then n x (x, y, z) float32 values; OUT: 64-bit words: the bits of min x, y, z
//                                       (float32), the bits of side (float64), then per point qx, qy, qz, key
//   codec_packet_host colour IN OUT     OUT: for s in 0..4, m in 0..255: stored, loaded (bytes); then for each quality 0..100 its shift
//   codec_packet_host mean IN OUT       IN: doubles (sum, count) pairs; OUT: the rounded means, 32-bit words
//   codec_packet_host decode IN OUT     IN: doubles bits, side, min x, y, z, n, then n keys; OUT: per key x, y, z (float32 bits), then the cellsize (float32 bits)
//   codec_packet_host validate IN OUT   IN: packets, each behind its length (u32); OUT: per packet a byte 1 (valid) / 0, a length byte and
//                                       the message; for a valid one then nleaves, total_bytes (u64 each)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "codec_terms.hpp"

using namespace cwipc_amd;

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> data;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + got);
    fclose(f);
    return data;
}

static void write_file(const char *path, const std::vector<uint8_t> &data) {
    FILE *f = fopen(path, "wb");
    if (!f) { perror(path); exit(2); }
    if (!data.empty() && fwrite(data.data(), 1, data.size(), f) != data.size()) { perror(path); exit(2); }
    fclose(f);
}

template <typename T>
static void put(std::vector<uint8_t> &out, T v) {
    uint8_t b[sizeof(T)];
    memcpy(b, &v, sizeof(T));
    out.insert(out.end(), b, b + sizeof(T));
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: codec_packet_host MODE IN OUT\n"); return 2; }
    const std::string mode = argv[1];
    const std::vector<uint8_t> raw = read_file(argv[2]);
    std::vector<double> in(raw.size() / 8);
    if (!in.empty()) memcpy(in.data(), raw.data(), in.size() * 8);
    std::vector<uint8_t> out;
    if (mode == "cells") {
        const int bits = (int)in[0];
        const size_t n = (size_t)in[1];
        std::vector<float> p(3 * n);
        for (size_t i = 0; i < 3 * n; i++) p[i] = (float)in[2 + i];
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t i = 0; i < n; i++)
            for (int a = 0; a < 3; a++) { mn[a] = fminf(mn[a], p[3 * i + a]); mx[a] = fmaxf(mx[a], p[3 * i + a]); }
        for (int a = 0; a < 3; a++) mn[a] = codec_min_canonical(mn[a]);
        const double side = codec_side(mn, mx);
        for (int a = 0; a < 3; a++) { uint32_t w; memcpy(&w, &mn[a], 4); put<uint64_t>(out, w); }
        { uint64_t w; memcpy(&w, &side, 8); put<uint64_t>(out, w); }
        for (size_t i = 0; i < n; i++) {
            uint32_t q[3], back[3];
            for (int a = 0; a < 3; a++) { q[a] = codec_cell(p[3 * i + a], mn[a], side, bits); put<uint64_t>(out, q[a]); }
            const uint64_t key = codec_key(q[0], q[1], q[2]);
            codec_unkey(key, back);
            if (back[0] != q[0] || back[1] != q[1] || back[2] != q[2]) { fprintf(stderr, "codec_unkey does not undo codec_key\n"); return 3; }
            put<uint64_t>(out, key);
        }
    } else if (mode == "colour") {
        for (int s = 0; s <= 4; s++)
            for (uint32_t m = 0; m < 256; m++) {
                const uint32_t v = codec_colour_store(m, s);
                put<uint8_t>(out, (uint8_t)v);
                put<uint8_t>(out, (uint8_t)codec_colour_load(v, s));
            }
        for (int q = 0; q <= 100; q++) put<uint8_t>(out, (uint8_t)codec_colour_shift(q));
    } else if (mode == "mean") {
        for (size_t i = 0; i + 1 < in.size(); i += 2) put<uint32_t>(out, codec_leaf_mean((uint64_t)in[i], (uint32_t)in[i + 1]));
    } else if (mode == "decode") {
        const int bits = (int)in[0];
        const double side = in[1];
        const float mn[3] = {(float)in[2], (float)in[3], (float)in[4]};
        const size_t n = (size_t)in[5];
        const double cell = codec_cellsize(side, bits);
        for (size_t i = 0; i < n; i++) {
            uint32_t q[3];
            codec_unkey((uint64_t)in[6 + i], q);
            for (int a = 0; a < 3; a++) { const float v = codec_position(mn[a], q[a], cell); uint32_t w; memcpy(&w, &v, 4); put<uint32_t>(out, w); }
        }
        { const float c = (float)cell; uint32_t w; memcpy(&w, &c, 4); put<uint32_t>(out, w); }
    } else if (mode == "validate") {
        size_t at = 0;
        while (at + 4 <= raw.size()) {
            uint32_t len;
            memcpy(&len, raw.data() + at, 4);
            at += 4;
            if (at + len > raw.size()) { fprintf(stderr, "bad input file\n"); return 2; }
            // a copy of exactly `len` bytes on the heap: a read one byte past the packet is the sanitizer's to report
            std::vector<uint8_t> packet(raw.begin() + (long)at, raw.begin() + (long)(at + len));
            at += len;
            CodecLayout l;
            const char *problem = codec_validate(packet.data(), packet.size(), l);
            const std::string msg = problem ? problem : "";
            put<uint8_t>(out, problem ? 0 : 1);
            put<uint8_t>(out, (uint8_t)msg.size());
            out.insert(out.end(), msg.begin(), msg.end());
            if (!problem) { put<uint64_t>(out, l.nleaves); put<uint64_t>(out, l.total_bytes); }
        }
    } else {
        fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_file(argv[3], out);
    return 0;
}
