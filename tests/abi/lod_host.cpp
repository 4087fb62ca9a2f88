// RULE L's host code (csrc/lod_terms.hpp) compiled stand-alone for tests/test_lod_host.py: built with
// -fsanitize=address,undefined -fno-sanitize-recover=all.  Every packet is handed over as a heap copy of exactly its length: a read
// one byte past it is the sanitizer's to report.
//   lod_host lod IN OUT     IN: records u32 bits, u32 length, the packet ("cwao" or "cwae"); OUT: per record a byte 1 and the cut packet
//                           behind its length (u32), or a byte 0, a length byte and the message
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lod_terms.hpp"

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
    uint32_t u32() {
        const std::vector<uint8_t> v = take(4);
        uint32_t w;
        memcpy(&w, v.data(), 4);
        return w;
    }
};

int main(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "lod") { fprintf(stderr, "usage: lod_host lod IN OUT\n"); return 2; }
    const std::vector<uint8_t> raw = read_file(argv[2]);
    Reader in{raw};
    std::vector<uint8_t> out;
    while (in.more()) {
        const int bits = (int)in.u32();
        const std::vector<uint8_t> packet = in.take(in.u32());
        std::vector<uint8_t> made;
        if (const char *problem = lod_convert(packet.data(), packet.size(), bits, made)) {
            const std::string msg = problem;
            put<uint8_t>(out, 0);
            put<uint8_t>(out, (uint8_t)msg.size());
            out.insert(out.end(), msg.begin(), msg.end());
            continue;
        }
        put<uint8_t>(out, 1);
        put<uint32_t>(out, (uint32_t)made.size());
        out.insert(out.end(), made.begin(), made.end());
    }
    write_file(argv[3], out);
    return 0;
}
