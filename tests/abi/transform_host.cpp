// RULE T's host code (csrc/transform_terms.hpp) compiled stand-alone for tests/test_transform_host.py: built with
// -fsanitize=address,undefined -fno-sanitize-recover=all.  Every packet is handed over as a heap copy of exactly its length: a read
// one byte past it is the sanitizer's to report.  Records are packets behind their lengths (u32); a result is a byte 1 and the packet
// behind its length (u32), or a byte 0, a length byte and the message.
//   transform_host pack IN OUT       records: u32 jpeg_quality, P ("cwao")   -> "cwat"
//   transform_host unpack IN OUT     records: T ("cwat")                      -> the "cwao" packet it stands for
//   transform_host validate IN OUT   records: T -> the container test: a byte 1, Q16, dc[3] (i32), nescapes[3], S (u32 each) and per
//                                    stream mode, payload bytes (u32 each)
//   transform_host terms IN OUT      records: u8 what, u64 a, i64 b, u64 c -> u64: 0 isqrt(a); 1 floor_div(b, c); 2 q16(b);
//                                    3 step(a, b, c)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "transform_terms.hpp"

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

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: transform_host MODE IN OUT\n"); return 2; }
    const std::string mode = argv[1];
    const std::vector<uint8_t> raw = read_file(argv[2]);
    Reader in{raw};
    std::vector<uint8_t> out;
    if (mode == "pack") {
        while (in.more()) {
            const uint32_t quality = in.get<uint32_t>();
            const std::vector<uint8_t> p = in.take(in.get<uint32_t>());
            std::vector<uint8_t> made;
            if (const char *problem = transform_pack(p.data(), p.size(), (int)quality, made)) { put_problem(out, problem); continue; }
            put_packet(out, made);
        }
    } else if (mode == "unpack") {
        while (in.more()) {
            const std::vector<uint8_t> t = in.take(in.get<uint32_t>());
            std::vector<uint8_t> made;
            if (const char *problem = transform_unpack(t.data(), t.size(), made)) { put_problem(out, problem); continue; }
            put_packet(out, made);
        }
    } else if (mode == "validate") {
        while (in.more()) {
            const std::vector<uint8_t> t = in.take(in.get<uint32_t>());
            TransformLayout e;
            if (const char *problem = transform_validate(t.data(), t.size(), e)) { put_problem(out, problem); continue; }
            if (e.cwao.nleaves && e.total_bytes != t.size()) { fprintf(stderr, "total_bytes differs from the length\n"); return 3; }
            put<uint8_t>(out, 1);
            put<uint32_t>(out, e.q16);
            for (int ch = 0; ch < 3; ch++) put<int32_t>(out, e.dc[ch]);
            for (int ch = 0; ch < 3; ch++) put<uint32_t>(out, e.nescapes[ch]);
            put<uint32_t>(out, (uint32_t)e.nstreams);
            for (int i = 0; i < e.nstreams; i++) { put<uint32_t>(out, e.stream[i].mode); put<uint32_t>(out, (uint32_t)e.stream[i].payload_bytes); }
        }
    } else if (mode == "terms") {
        while (in.more()) {
            const uint8_t what = in.get<uint8_t>();
            const uint64_t a = in.get<uint64_t>();
            const int64_t b = in.get<int64_t>();
            const uint64_t c = in.get<uint64_t>();
            uint64_t r = 0;
            if (what == 0) r = transform_isqrt(a);
            else if (what == 1) r = (uint64_t)transform_floor_div(b, (int64_t)c);
            else if (what == 2) r = transform_q16((int)b);
            else if (what == 3) r = transform_step((uint32_t)a, (uint32_t)b, (uint32_t)c);
            else { fprintf(stderr, "unknown term\n"); return 2; }
            put<uint64_t>(out, r);
        }
    } else {
        fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_file(argv[3], out);
    return 0;
}
