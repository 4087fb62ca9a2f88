// RULE P's host code (csrc/inter_terms.hpp) compiled stand-alone for tests/test_inter_host.py: built with
// -fsanitize=address,undefined -fno-sanitize-recover=all.  Every packet is handed over as a heap copy of exactly its length: a read
// one byte past it is the sanitizer's to report.  Records are packets behind their lengths (u32); a result is a byte 1 and the packet
// behind its length (u32), or a byte 0, a length byte and the message.
//   inter_host pack IN OUT       records: u32 gop_index, R, P ("cwao")        -> diff(P, R)
//   inter_host unpack IN OUT     records: R ("cwao"; length 0: none), D        -> apply(D, R)
//   inter_host validate IN OUT   records: R ("cwao"; length 0: the packet alone is looked at), D -> the container test: a byte 1, kind, nadded,
//                                S (u32 each) and per stream mode, payload bytes (u32 each)
//   inter_host cube IN OUT       records: f32 mn[3], f64 side, f32 exp_factor, f32 lo[3], f32 hi[3] -> f32 mn'[3], f64 side', u8 contained
//                                (lo, hi in the expanded cube)
//   inter_host sequence IN OUT   u32 gop_size, then per frame a byte: bit 0 empty, bit 1 contained -> per frame u8 boundary before it, u8 kind,
//                                u32 gop_index
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "inter_terms.hpp"

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

static void put_problem(std::vector<uint8_t> &out, const char *problem) {
    const std::string msg = problem;
    put<uint8_t>(out, 0);
    put<uint8_t>(out, (uint8_t)msg.size());
    out.insert(out.end(), msg.begin(), msg.end());
}

static void put_packet(std::vector<uint8_t> &out, const std::vector<uint8_t> &made) {
    put<uint8_t>(out, 1);
    put<uint32_t>(out, (uint32_t)made.size());
    out.insert(out.end(), made.begin(), made.end());
}

struct Reader {
    const std::vector<uint8_t> &raw;
    size_t at = 0;
    bool more() const { return at < raw.size(); }
    std::vector<uint8_t> take(size_t n) {
        if (at + n > raw.size()) { fprintf(stderr, "bad input file\n"); exit(2); }
        std::vector<uint8_t> v(raw.begin() + (long)at, raw.begin() + (long)(at + n));
        at += n;
        return v;
    }
    template <typename T>
    T get() {
        const std::vector<uint8_t> v = take(sizeof(T));
        T w;
        memcpy(&w, v.data(), sizeof(T));
        return w;
    }
};

static bool reference_of(const std::vector<uint8_t> &r, InterReference &ref) {
    CodecLayout l;
    if (codec_validate(r.data(), r.size(), l)) { fprintf(stderr, "the reference of a record is not a valid packet\n"); exit(2); }
    ref.timestamp = l.timestamp;
    ref.nleaves = l.nleaves;
    ref.bits = l.bits;
    ref.colour_bits = l.colour_bits;
    memcpy(ref.mn, l.mn, 12);
    ref.side = l.side;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: inter_host MODE IN OUT\n"); return 2; }
    const std::string mode = argv[1];
    const std::vector<uint8_t> raw = read_file(argv[2]);
    Reader in{raw};
    std::vector<uint8_t> out;
    if (mode == "pack") {
        while (in.more()) {
            const uint32_t gop_index = in.get<uint32_t>();
            const std::vector<uint8_t> r = in.take(in.get<uint32_t>()), p = in.take(in.get<uint32_t>());
            std::vector<uint8_t> made;
            if (const char *problem = inter_pack(r.data(), r.size(), p.data(), p.size(), gop_index, made)) { put_problem(out, problem); continue; }
            put_packet(out, made);
        }
    } else if (mode == "unpack") {
        while (in.more()) {
            const std::vector<uint8_t> r = in.take(in.get<uint32_t>()), d = in.take(in.get<uint32_t>());
            std::vector<uint8_t> made;
            if (const char *problem = inter_unpack(r.empty() ? nullptr : r.data(), r.size(), d.data(), d.size(), made)) { put_problem(out, problem); continue; }
            put_packet(out, made);
        }
    } else if (mode == "validate") {
        while (in.more()) {
            const std::vector<uint8_t> r = in.take(in.get<uint32_t>()), d = in.take(in.get<uint32_t>());
            InterReference ref;
            const bool held = !r.empty() && reference_of(r, ref);
            InterLayout e;
            if (const char *problem = inter_validate(d.data(), d.size(), held ? &ref : nullptr, e)) { put_problem(out, problem); continue; }
            if (e.total_bytes != d.size()) { fprintf(stderr, "total_bytes differs from the length\n"); return 3; }
            put<uint8_t>(out, 1);
            put<uint32_t>(out, e.kind);
            put<uint32_t>(out, e.nadded);
            put<uint32_t>(out, (uint32_t)e.nstreams);
            for (int i = 0; i < e.nstreams; i++) { put<uint32_t>(out, e.stream[i].mode); put<uint32_t>(out, (uint32_t)e.stream[i].payload_bytes); }
        }
    } else if (mode == "cube") {
        while (in.more()) {
            float mn[3], lo[3], hi[3], grown_mn[3];
            for (int a = 0; a < 3; a++) mn[a] = in.get<float>();
            const double side = in.get<double>();
            const float exp_factor = in.get<float>();
            for (int a = 0; a < 3; a++) lo[a] = in.get<float>();
            for (int a = 0; a < 3; a++) hi[a] = in.get<float>();
            double grown = 0;
            inter_expand_cube(mn, side, exp_factor, grown_mn, grown);
            for (int a = 0; a < 3; a++) put<float>(out, grown_mn[a]);
            put<double>(out, grown);
            put<uint8_t>(out, inter_contained(lo, hi, grown_mn, grown) ? 1 : 0);
        }
    } else if (mode == "sequence") {
        InterSequence seq;
        seq.gop_size = (int)in.get<uint32_t>();
        while (in.more()) {
            const uint8_t frame = in.get<uint8_t>();
            put<uint8_t>(out, seq.at_gop_boundary() ? 1 : 0);
            uint32_t gop_index = 0;
            const uint32_t kind = seq.next((frame & 1u) != 0, (frame & 2u) != 0, gop_index);
            put<uint8_t>(out, (uint8_t)kind);
            put<uint32_t>(out, gop_index);
        }
    } else {
        fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_file(argv[3], out);
    return 0;
}
