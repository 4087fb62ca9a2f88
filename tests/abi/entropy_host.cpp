// RULE E's host code (csrc/entropy_terms.hpp) compiled stand-alone for tests/test_entropy_host.py: built with
// -fsanitize=address,undefined -fno-sanitize-recover=all.  Every packet is handed over as a heap copy of exactly its length: a read
// one byte past it is the sanitizer's to report.
//   entropy_host pack IN OUT        IN: "cwao" packets, each behind its length (u32); OUT: per packet a byte 1 and the "cwae" packet behind
//                                   its length (u32), or a byte 0, a length byte and the message
//   entropy_host unpack IN OUT      the same from "cwae" to "cwao": the container test, the blocks' integrity, the occupancy rules
//   entropy_host validate IN OUT    the container test alone: per packet a byte 1, then S (u32) and per stream mode, payload bytes (u32 each);
//                                   or a byte 0, a length byte and the message
//   entropy_host normalise IN OUT   IN: sets of 256 counts (u32); OUT: per set f[256] (u16)
//   entropy_host encode IN OUT      IN: records u32 m, u16 f[256], m symbol bytes; OUT: per record u32 bytes and the block
//   entropy_host decode IN OUT      IN: records u32 m, u16 f[256], u32 bytes, the block; OUT: per record a byte 1 (intact) / 0 and m symbol bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "entropy_terms.hpp"

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
    if (argc != 4) { fprintf(stderr, "usage: entropy_host MODE IN OUT\n"); return 2; }
    const std::string mode = argv[1];
    const std::vector<uint8_t> raw = read_file(argv[2]);
    Reader in{raw};
    std::vector<uint8_t> out;
    if (mode == "pack" || mode == "unpack") {
        while (in.more()) {
            const std::vector<uint8_t> packet = in.take(in.u32());
            std::vector<uint8_t> made;
            const char *problem = mode == "pack" ? entropy_pack(packet.data(), packet.size(), made) : entropy_unpack(packet.data(), packet.size(), made);
            if (problem) { put_problem(out, problem); continue; }
            put<uint8_t>(out, 1);
            put<uint32_t>(out, (uint32_t)made.size());
            out.insert(out.end(), made.begin(), made.end());
        }
    } else if (mode == "validate") {
        while (in.more()) {
            const std::vector<uint8_t> packet = in.take(in.u32());
            EntropyLayout e;
            if (const char *problem = entropy_validate(packet.data(), packet.size(), e)) { put_problem(out, problem); continue; }
            if (e.total_bytes != packet.size()) { fprintf(stderr, "total_bytes differs from the length\n"); return 3; }
            put<uint8_t>(out, 1);
            put<uint32_t>(out, (uint32_t)e.nstreams);
            for (int i = 0; i < e.nstreams; i++) { put<uint32_t>(out, e.stream[i].mode); put<uint32_t>(out, (uint32_t)e.stream[i].payload_bytes); }
        }
    } else if (mode == "normalise") {
        while (in.more()) {
            const std::vector<uint8_t> set = in.take(1024);
            uint32_t c[256];
            uint16_t f[256];
            memcpy(c, set.data(), 1024);
            entropy_normalise(c, f);
            for (int i = 0; i < 256; i++) put<uint16_t>(out, f[i]);
        }
    } else if (mode == "encode") {
        while (in.more()) {
            const uint32_t m = in.u32();
            const std::vector<uint8_t> table = in.take(512), sym = in.take(m);
            uint16_t f[256], cum[256];
            memcpy(f, table.data(), 512);
            entropy_cumulate(f, cum);
            uint32_t states[ENTROPY_LANES];
            std::vector<uint16_t> words;
            entropy_block_encode(sym.data(), m, f, cum, states, words);
            const uint32_t bytes = entropy_block_bytes((uint32_t)words.size());
            put<uint32_t>(out, bytes);
            for (uint32_t l = 0; l < ENTROPY_LANES; l++) put<uint32_t>(out, states[l]);
            for (uint16_t w : words) put<uint16_t>(out, w);
            if (words.size() & 1u) put<uint16_t>(out, 0);
        }
    } else if (mode == "decode") {
        while (in.more()) {
            const uint32_t m = in.u32();
            const std::vector<uint8_t> table = in.take(512);
            const uint32_t bytes = in.u32();
            const std::vector<uint8_t> block = in.take(bytes);
            if (m < 1 || m > ENTROPY_BLOCK || bytes < ENTROPY_STATES_BYTES || (bytes & 3u)) { fprintf(stderr, "bad record\n"); return 2; }
            uint16_t f[256], cum[256];
            memcpy(f, table.data(), 512);
            entropy_cumulate(f, cum);
            std::vector<uint8_t> sym(m, 0);
            put<uint8_t>(out, entropy_block_decode(block.data(), bytes, m, f, cum, sym.data()) ? 1 : 0);
            out.insert(out.end(), sym.begin(), sym.end());
        }
    } else {
        fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_file(argv[3], out);
    return 0;
}
