// entropy_terms.hpp -- RULE E, the entropy-coded form of the octree codec's packets (the rule in full: hip_ext.h; its numpy
// restatement: tests/entropy_model.py).  A "cwae" packet stands for exactly one valid "cwao" packet (RULE C, codec_terms.hpp): the same
// header, and every stream of the body either as it is (raw) or coded with a 64-lane interleaved rANS.  Compiles for host and device:
// kernels_entropy.hip, the codec_*.cpp files and the stand-alone host program of the tests (tests/abi/entropy_host.cpp) include this one text.
// The per-symbol steps, the slot search, the bounded word read and the end-of-block test are the very functions the kernels call; the
// block loops below run them lane by lane where a kernel runs them on the 64 lanes of a wave.  The normalisation is serial here and
// runs on a wave in the kernel (the same steps, its maxima taken across lanes); the GPU tests hold the two to each other.
#pragma once

#include "codec_terms.hpp"

#include <vector>

namespace cwipc_amd {

constexpr uint32_t ENTROPY_MAGIC = 0x65617763u;   // the bytes c w a e
constexpr uint32_t ENTROPY_VERSION = 1u;
constexpr uint32_t ENTROPY_BLOCK = 4096u;         // symbols per block
constexpr uint32_t ENTROPY_LANES = 64u;           // interleaved coders per block
constexpr uint32_t ENTROPY_M = 4096u;             // the frequencies of a stream sum to this (12 bits)
constexpr uint32_t ENTROPY_LOW = 1u << 16;        // a state lies in [2^16, 2^32)
constexpr uint32_t ENTROPY_STATES_BYTES = 4u * ENTROPY_LANES;
constexpr uint32_t ENTROPY_TABLE_BYTES = 512u;    // u16 f[256]
constexpr int ENTROPY_MAX_STREAMS = CODEC_MAX_BITS + 4;

// The first three are RULE E's streams, read from a packet's body.  The last two are plain byte planes, one byte per symbol, coded
// without prediction (RULE P's streams, inter_terms.hpp): BYTES is raw as it is, BITS is raw packed at colour-bits per symbol.
enum EntropyKind : uint32_t { ENTROPY_OCCUPANCY = 0, ENTROPY_COLOUR = 1, ENTROPY_TILE = 2, ENTROPY_BYTES = 3, ENTROPY_BITS = 4 };
CW_CODEC_HD inline bool entropy_kind_packed(uint32_t kind) { return kind == ENTROPY_COLOUR || kind == ENTROPY_BITS; }

// ---------------------------------------------------------------------------
// the arithmetic (host and device)
// ---------------------------------------------------------------------------
// f[] from the 256 counts of a stream (at least one count is not 0); 64-bit products
CW_CODEC_HD inline void entropy_normalise(const uint32_t c[256], uint16_t f[256]) {
    uint64_t total = 0;
    for (int i = 0; i < 256; i++) total += c[i];
    int sum = 0, best = 0;
    for (int i = 0; i < 256; i++) {
        uint32_t v = 0;
        if (c[i]) {
            v = (uint32_t)(((uint64_t)c[i] * ENTROPY_M) / total);
            if (v < 1u) v = 1u;
        }
        f[i] = (uint16_t)v;
        sum += (int)v;
        if (c[i] > c[best]) best = i;   // the largest count, the lowest symbol on ties
    }
    int d = (int)ENTROPY_M - sum;
    if (d > 0) f[best] = (uint16_t)(f[best] + d);
    for (; d < 0; d++) {
        int top = 0;
        for (int i = 1; i < 256; i++)
            if (f[i] > f[top]) top = i;   // the largest f, the lowest symbol on ties; above 1 (256 symbols sum to more than 4096)
        f[top] = (uint16_t)(f[top] - 1);
    }
}

CW_CODEC_HD inline void entropy_cumulate(const uint16_t f[256], uint16_t cum[256]) {
    uint32_t at = 0;
    for (int i = 0; i < 256; i++) { cum[i] = (uint16_t)at; at += f[i]; }
}

// One symbol into a lane's state (f > 0).  True: `word` is emitted BEFORE the symbol goes in.
CW_CODEC_HD inline bool entropy_put(uint32_t &x, uint32_t f, uint32_t cum, uint16_t &word) {
    const bool emit = (uint64_t)x >= ((uint64_t)f << 20);
    if (emit) {
        word = (uint16_t)(x & 0xffffu);
        x >>= 16;
    }
    x = (x / f) * ENTROPY_M + (x % f) + cum;
    return emit;
}

// The largest s with cum[s] <= slot: in 0..255 for ANY table, and with f[s] > 0 when cum is the prefix sum of an f that sums to 4096.
CW_CODEC_HD inline uint32_t entropy_find(const uint16_t *cum, uint32_t slot) {
    uint32_t s = 0;
    for (uint32_t step = 128; step; step >>= 1)
        if ((uint32_t)cum[s + step] <= slot) s += step;
    return s;
}

// One symbol out of a lane's state.
CW_CODEC_HD inline uint32_t entropy_get(uint32_t &x, const uint16_t *f, const uint16_t *cum) {
    const uint32_t slot = x & (ENTROPY_M - 1u);
    const uint32_t s = entropy_find(cum, slot);
    x = (uint32_t)f[s] * (x >> 12) + slot - (uint32_t)cum[s];
    return s;
}

// Word `at` of a block of `count` word slots: a read past the block gives 0 and raises the flag.
CW_CODEC_HD inline uint32_t entropy_word(const uint8_t *words, uint32_t count, uint32_t at, uint32_t &past) {
    if (at >= count) {
        past = 1u;
        return 0u;
    }
    return (uint32_t)words[2u * at] | ((uint32_t)words[2u * at + 1u] << 8);
}

// After the decoder's last round: all 64 states back at 2^16, and the cursor at the end of the words (W word slots: the cursor is W,
// or W - 1 with the last slot, the padding word, being 0).
CW_CODEC_HD inline bool entropy_cursor_at_end(const uint8_t *words, uint32_t count, uint32_t cursor) {
    if (cursor == count) return true;
    return cursor + 1u == count && words[2u * cursor] == 0 && words[2u * cursor + 1u] == 0;
}

CW_CODEC_HD inline uint32_t entropy_block_count(uint64_t symbols) { return (uint32_t)((symbols + ENTROPY_BLOCK - 1u) / ENTROPY_BLOCK); }
CW_CODEC_HD inline uint32_t entropy_block_symbols(uint64_t symbols, uint32_t block) {
    const uint64_t left = symbols - (uint64_t)block * ENTROPY_BLOCK;
    return left < ENTROPY_BLOCK ? (uint32_t)left : ENTROPY_BLOCK;
}
CW_CODEC_HD inline uint32_t entropy_block_bytes(uint32_t words) { return ENTROPY_STATES_BYTES + ((2u * words + 3u) & ~3u); }

// ---------------------------------------------------------------------------
// the container
// ---------------------------------------------------------------------------
struct EntropyStream {
    uint32_t kind = 0, which = 0;      // occupancy: the depth; colour: the channel
    uint32_t symbols = 0, nblocks = 0;
    uint32_t children = 0;             // occupancy: the bits its bytes must hold (the node count of its depth)
    uint64_t raw_bytes = 0;            // the raw payload without its padding
    uint32_t mode = 0;
    uint64_t payload_offset = 0, payload_bytes = 0;
};

struct EntropyLayout {
    CodecLayout cwao;                  // the packet this one stands for (offsets and sizes of the "cwao" form)
    int nstreams = 0;
    EntropyStream stream[ENTROPY_MAX_STREAMS];
    uint64_t directory_offset = 0;     // where the u32 S lies
    uint64_t total_bytes = 0;
};

// The streams a header implies, in RULE E's order; returns S.
inline int entropy_streams(const CodecLayout &l, EntropyStream s[ENTROPY_MAX_STREAMS]) {
    int n = 0;
    if (!l.nleaves) return 0;
    for (int d = 0; d < l.bits; d++) {
        EntropyStream e;
        e.kind = ENTROPY_OCCUPANCY;
        e.which = (uint32_t)d;
        e.symbols = d == 0 ? 1u : l.nodes[d - 1];
        e.children = l.nodes[d];
        e.raw_bytes = e.symbols;
        s[n++] = e;
    }
    for (int ch = 0; ch < 3; ch++) {
        EntropyStream e;
        e.kind = ENTROPY_COLOUR;
        e.which = (uint32_t)ch;
        e.symbols = l.nleaves;
        e.raw_bytes = ((uint64_t)l.nleaves * (uint64_t)l.colour_bits + 7u) / 8u;
        s[n++] = e;
    }
    if (l.tile_mode == 1) {
        EntropyStream e;
        e.kind = ENTROPY_TILE;
        e.symbols = l.nleaves;
        e.raw_bytes = l.nleaves;
        s[n++] = e;
    }
    for (int i = 0; i < n; i++) s[i].nblocks = entropy_block_count(s[i].symbols);
    return n;
}

// where depth d's occupancy bytes start, relative to the first occupancy byte
inline uint64_t entropy_depth_offset(const CodecLayout &l, int d) {
    uint64_t at = 0;
    for (int i = 0; i < d; i++) at += i == 0 ? 1u : l.nodes[i - 1];
    return at;
}

// `width` bits at bit `bit` of a plane of `plane_bytes` bytes, LSB first (width <= 8)
CW_CODEC_HD inline uint32_t entropy_bits_at(const uint8_t *plane, uint64_t plane_bytes, uint64_t bit, int width) {
    const uint64_t byte = bit >> 3;
    uint32_t v = byte < plane_bytes ? plane[byte] : 0u;
    if (byte + 1 < plane_bytes) v |= (uint32_t)plane[byte + 1] << 8;
    return (v >> (uint32_t)(bit & 7u)) & ((1u << width) - 1u);
}
inline void entropy_bits_put(uint8_t *plane, uint64_t bit, int width, uint32_t value) {
    const uint32_t v = value << (uint32_t)(bit & 7u);
    plane[bit >> 3] |= (uint8_t)v;
    if (((bit & 7u) + (uint64_t)width) > 8u) plane[(bit >> 3) + 1] |= (uint8_t)(v >> 8);
}

// The directory at `directory_offset` (the u32 S, the S entries) and the payloads behind it, held to the counts of `stream[]` (kind,
// symbols, nblocks, raw_bytes, children filled): mode, payload_offset and payload_bytes are filled in, `total_bytes` is where the
// last payload ends, which must be `len`.  The coded blocks are not decoded here.  Nothing outside [p, p + len) is read.
inline const char *entropy_validate_streams(const uint8_t *p, size_t len, uint64_t directory_offset, int nstreams, EntropyStream *stream, int colour_bits,
                                            uint64_t &total_bytes) {
    if ((uint64_t)len < directory_offset + 4u) return "truncated stream count";
    if (codec_read<uint32_t>(p + directory_offset) != (uint32_t)nstreams) return "stream count differs from the header's";
    uint64_t at = directory_offset + 4u + 8u * (uint64_t)nstreams;
    if ((uint64_t)len < at) return "truncated directory";
    for (int i = 0; i < nstreams; i++) {
        EntropyStream &s = stream[i];
        s.mode = codec_read<uint32_t>(p + directory_offset + 4u + 8u * (uint64_t)i);
        s.payload_bytes = codec_read<uint32_t>(p + directory_offset + 8u + 8u * (uint64_t)i);
        if (s.mode > 1u) return "unknown stream mode";
        if (s.mode == 0u) {
            if (s.payload_bytes != codec_pad4(s.raw_bytes)) return "raw payload size differs from the header's counts";
        } else {
            if (s.symbols < ENTROPY_BLOCK) return "coded stream of fewer than 4096 symbols";
            if (s.payload_bytes & 3u) return "coded payload size is not a multiple of 4";
            if (s.payload_bytes < ENTROPY_TABLE_BYTES + (uint64_t)s.nblocks * (4u + ENTROPY_STATES_BYTES)) return "coded payload too small for its blocks";
            if (s.payload_bytes >= codec_pad4(s.raw_bytes)) return "coded payload is not smaller than the raw one";
        }
        s.payload_offset = at;
        at += s.payload_bytes;
    }
    total_bytes = at;
    if ((uint64_t)len < total_bytes) return "truncated packet";
    if ((uint64_t)len > total_bytes) return "bytes behind the packet";
    for (int i = 0; i < nstreams; i++) {
        const EntropyStream &s = stream[i];
        const uint8_t *q = p + s.payload_offset;
        if (s.mode == 0u) {
            if (s.kind == ENTROPY_OCCUPANCY) {
                uint64_t children = 0;
                for (uint64_t k = 0; k < s.symbols; k++) {
                    if (q[k] == 0) return "occupancy byte is 0";
                    children += (uint64_t)__builtin_popcount(q[k]);
                }
                if (children != s.children) return "occupancy bits differ from the node count";
            } else if (entropy_kind_packed(s.kind)) {
                const uint64_t bit_count = (uint64_t)s.symbols * (uint64_t)colour_bits;
                if ((bit_count & 7u) && (q[s.raw_bytes - 1] >> (bit_count & 7u))) return "padding is not 0";
            }
            for (uint64_t k = s.raw_bytes; k < s.payload_bytes; k++)
                if (q[k] != 0) return "padding is not 0";
            continue;
        }
        uint32_t sum = 0;
        for (int k = 0; k < 256; k++) sum += codec_read<uint16_t>(q + 2 * k);
        if (sum != ENTROPY_M) return "frequencies do not sum to 4096";
        if (s.kind == ENTROPY_OCCUPANCY && codec_read<uint16_t>(q) != 0) return "occupancy byte 0 has a frequency";
        if (entropy_kind_packed(s.kind))
            for (int k = 1 << colour_bits; k < 256; k++)
                if (codec_read<uint16_t>(q + 2 * k) != 0) return "a colour value above its bits has a frequency";
        uint64_t blocks = 0;
        for (uint32_t k = 0; k < s.nblocks; k++) {
            const uint32_t bytes = codec_read<uint32_t>(q + ENTROPY_TABLE_BYTES + 4u * (uint64_t)k);
            if (bytes & 3u) return "block size is not a multiple of 4";
            if (bytes < ENTROPY_STATES_BYTES) return "block smaller than its states";
            if (bytes > ENTROPY_STATES_BYTES + 2u * ENTROPY_BLOCK) return "block larger than a word per symbol";
            blocks += bytes;
        }
        if (blocks != s.payload_bytes - ENTROPY_TABLE_BYTES - 4u * (uint64_t)s.nblocks) return "block sizes differ from the payload size";
    }
    return nullptr;
}

// The container test: host code, one pass over the directory, the tables and the raw streams; the coded blocks are not decoded here.
// nullptr: the container is right and `out` filled; otherwise why not.  Nothing outside [p, p + len) is read.
inline const char *entropy_validate(const uint8_t *p, size_t len, EntropyLayout &out) {
    EntropyLayout e;
    CodecLayout &l = e.cwao;
    if (const char *problem = codec_validate_header(p, len, ENTROPY_MAGIC, l)) return problem;
    e.directory_offset = CODEC_HEADER_BYTES + 4u * (uint64_t)l.bits;
    e.nstreams = entropy_streams(l, e.stream);
    if (const char *problem = entropy_validate_streams(p, len, e.directory_offset, e.nstreams, e.stream, l.colour_bits, e.total_bytes)) return problem;
    out = e;
    return nullptr;
}

// ---------------------------------------------------------------------------
// blocks on the host: the kernels' arithmetic, lane by lane
// ---------------------------------------------------------------------------
// m symbols -> the 64 states the decoder starts from and the words in the order the decoder takes them
inline void entropy_block_encode(const uint8_t *sym, uint32_t m, const uint16_t f[256], const uint16_t cum[256], uint32_t states[ENTROPY_LANES],
                                 std::vector<uint16_t> &words) {
    for (uint32_t l = 0; l < ENTROPY_LANES; l++) states[l] = ENTROPY_LOW;
    std::vector<uint16_t> emitted;
    const uint32_t rounds = (m + ENTROPY_LANES - 1u) / ENTROPY_LANES;
    for (uint32_t r = rounds; r-- > 0;)
        for (uint32_t l = ENTROPY_LANES; l-- > 0;) {
            const uint32_t j = ENTROPY_LANES * r + l;
            if (j >= m) continue;
            uint16_t w = 0;
            if (entropy_put(states[l], f[sym[j]], cum[sym[j]], w)) emitted.push_back(w);
        }
    words.assign(emitted.rbegin(), emitted.rend());
}

// A block of `bytes` bytes (a multiple of 4, at least 256) -> m symbols into out[0 .. m).  True: the block is intact.  For ANY bytes
// nothing outside [block, block + bytes) is read and nothing outside out[0 .. m) is written.
inline bool entropy_block_decode(const uint8_t *block, uint32_t bytes, uint32_t m, const uint16_t f[256], const uint16_t cum[256], uint8_t *out) {
    const uint8_t *words = block + ENTROPY_STATES_BYTES;
    const uint32_t count = (bytes - ENTROPY_STATES_BYTES) / 2u;
    uint32_t x[ENTROPY_LANES], bad = 0, cursor = 0;
    for (uint32_t l = 0; l < ENTROPY_LANES; l++) {
        x[l] = codec_read<uint32_t>(block + 4u * l);
        if (x[l] < ENTROPY_LOW) bad = 1u;
    }
    const uint32_t rounds = (m + ENTROPY_LANES - 1u) / ENTROPY_LANES;
    for (uint32_t r = 0; r < rounds; r++) {
        for (uint32_t l = 0; l < ENTROPY_LANES && ENTROPY_LANES * r + l < m; l++) out[ENTROPY_LANES * r + l] = (uint8_t)entropy_get(x[l], f, cum);
        for (uint32_t l = 0; l < ENTROPY_LANES && ENTROPY_LANES * r + l < m; l++)
            if (x[l] < ENTROPY_LOW) x[l] = (x[l] << 16) | entropy_word(words, count, cursor++, bad);
    }
    for (uint32_t l = 0; l < ENTROPY_LANES; l++)
        if (x[l] != ENTROPY_LOW) bad = 1u;
    if (!bad && !entropy_cursor_at_end(words, count, cursor)) bad = 1u;
    return bad == 0u;
}

// ---------------------------------------------------------------------------
// whole packets on the host
// ---------------------------------------------------------------------------
// the plain values of stream s of the valid "cwao" packet p
inline void entropy_stream_values(const uint8_t *p, const CodecLayout &l, const EntropyStream &s, std::vector<uint8_t> &v) {
    v.resize(s.symbols);
    if (s.kind == ENTROPY_OCCUPANCY) {
        memcpy(v.data(), p + l.occupancy_offset + entropy_depth_offset(l, (int)s.which), s.symbols);
    } else if (s.kind == ENTROPY_TILE) {
        memcpy(v.data(), p + l.tile_offset, s.symbols);
    } else {
        const int cb = l.colour_bits;
        for (uint64_t j = 0; j < s.symbols; j++)
            v[j] = (uint8_t)entropy_bits_at(p + l.colour_offset, l.colour_bytes, (3u * j + s.which) * (uint64_t)cb, cb);
    }
}

// The payload of stream s from its plain values v (one a byte) and its mode, by RULE E: raw (a packed kind at cb bits a value), or
// coded where the stream has at least 4096 symbols and comes out strictly smaller.  Only ENTROPY_COLOUR is predicted.
inline void entropy_make_payload(EntropyStream &s, const std::vector<uint8_t> &v, int cb, std::vector<uint8_t> &payload) {
    std::vector<uint8_t> raw((size_t)codec_pad4(s.raw_bytes), 0);
    if (entropy_kind_packed(s.kind)) {
        for (uint64_t j = 0; j < s.symbols; j++) entropy_bits_put(raw.data(), j * (uint64_t)cb, cb, v[j]);
    } else {
        memcpy(raw.data(), v.data(), s.symbols);
    }
    s.mode = 0;
    if (s.symbols >= ENTROPY_BLOCK) {
        std::vector<uint8_t> sym = v;
        if (s.kind == ENTROPY_COLOUR) {
            const uint32_t mask = (1u << cb) - 1u;
            for (uint64_t j = 0; j < s.symbols; j++)
                if (j % ENTROPY_BLOCK) sym[j] = (uint8_t)(((uint32_t)v[j] - (uint32_t)v[j - 1]) & mask);
        }
        uint32_t counts[256] = {0};
        for (uint8_t b : sym) counts[b]++;
        uint16_t f[256], cum[256];
        entropy_normalise(counts, f);
        entropy_cumulate(f, cum);
        std::vector<uint8_t> coded(ENTROPY_TABLE_BYTES + 4u * (size_t)s.nblocks, 0);
        memcpy(coded.data(), f, ENTROPY_TABLE_BYTES);
        std::vector<uint16_t> words;
        for (uint32_t k = 0; k < s.nblocks; k++) {
            uint32_t states[ENTROPY_LANES];
            entropy_block_encode(sym.data() + (size_t)k * ENTROPY_BLOCK, entropy_block_symbols(s.symbols, k), f, cum, states, words);
            const uint32_t bytes = entropy_block_bytes((uint32_t)words.size());
            memcpy(coded.data() + ENTROPY_TABLE_BYTES + 4u * (size_t)k, &bytes, 4);
            const size_t at = coded.size();
            coded.resize(at + bytes, 0);
            memcpy(coded.data() + at, states, ENTROPY_STATES_BYTES);
            if (!words.empty()) memcpy(coded.data() + at + ENTROPY_STATES_BYTES, words.data(), 2u * words.size());
        }
        if (coded.size() < raw.size()) {
            s.mode = 1;
            raw.swap(coded);
        }
    }
    payload.swap(raw);
}

// The plain values of stream s (mode and sizes as entropy_validate_streams() left them) from its payload q: nullptr and v filled, or
// why the stream is refused: a block that is not intact, or, for occupancy, RULE C's two conditions.
inline const char *entropy_read_payload(const uint8_t *q, const EntropyStream &s, int cb, std::vector<uint8_t> &v) {
    v.assign(s.symbols, 0);
    if (s.mode == 0u) {
        if (entropy_kind_packed(s.kind)) {
            for (uint64_t j = 0; j < s.symbols; j++) v[j] = (uint8_t)entropy_bits_at(q, s.raw_bytes, j * (uint64_t)cb, cb);
        } else {
            memcpy(v.data(), q, s.symbols);
        }
        return nullptr;
    }
    uint16_t f[256], cum[256];
    memcpy(f, q, ENTROPY_TABLE_BYTES);
    entropy_cumulate(f, cum);
    const uint8_t *block = q + ENTROPY_TABLE_BYTES + 4u * (size_t)s.nblocks;
    for (uint32_t k = 0; k < s.nblocks; k++) {
        const uint32_t bytes = codec_read<uint32_t>(q + ENTROPY_TABLE_BYTES + 4u * (size_t)k);
        if (!entropy_block_decode(block, bytes, entropy_block_symbols(s.symbols, k), f, cum, v.data() + (size_t)k * ENTROPY_BLOCK))
            return "entropy-coded block is not intact";
        block += bytes;
    }
    if (s.kind == ENTROPY_COLOUR) {
        const uint32_t mask = (1u << cb) - 1u;
        for (uint64_t j = 0; j < s.symbols; j++)
            if (j % ENTROPY_BLOCK) v[j] = (uint8_t)(((uint32_t)v[j] + (uint32_t)v[j - 1]) & mask);
    } else if (s.kind == ENTROPY_OCCUPANCY) {
        uint64_t children = 0;
        for (uint8_t b : v) {
            if (b == 0) return "occupancy byte is 0";
            children += (uint64_t)__builtin_popcount(b);
        }
        if (children != s.children) return "occupancy bits differ from the node count";
    }
    return nullptr;
}

// "cwao" -> "cwae".  nullptr and `out` filled, or why the input is not a valid packet.
inline const char *entropy_pack(const uint8_t *p, size_t len, std::vector<uint8_t> &out) {
    CodecLayout l;
    if (const char *problem = codec_validate(p, len, l)) return problem;
    EntropyStream streams[ENTROPY_MAX_STREAMS];
    const int S = entropy_streams(l, streams);
    std::vector<std::vector<uint8_t>> payload((size_t)S);
    std::vector<uint8_t> v;
    for (int i = 0; i < S; i++) {
        entropy_stream_values(p, l, streams[i], v);
        entropy_make_payload(streams[i], v, l.colour_bits, payload[(size_t)i]);
    }
    const size_t head = CODEC_HEADER_BYTES + 4u * (size_t)l.bits;
    out.assign(p, p + head);
    const uint32_t magic = ENTROPY_MAGIC, version = ENTROPY_VERSION, count = (uint32_t)S;
    memcpy(out.data(), &magic, 4);
    memcpy(out.data() + 4, &version, 4);
    out.resize(head + 4u + 8u * (size_t)S, 0);
    memcpy(out.data() + head, &count, 4);
    for (int i = 0; i < S; i++) {
        const uint32_t entry[2] = {streams[i].mode, (uint32_t)payload[(size_t)i].size()};
        memcpy(out.data() + head + 4u + 8u * (size_t)i, entry, 8);
    }
    for (int i = 0; i < S; i++) out.insert(out.end(), payload[(size_t)i].begin(), payload[(size_t)i].end());
    return nullptr;
}

// "cwae" -> the "cwao" packet it stands for.  nullptr and `out` filled, or why the packet is refused: the container test, then for
// every coded stream its blocks' integrity and, for occupancy, RULE C's two conditions.
inline const char *entropy_unpack(const uint8_t *p, size_t len, std::vector<uint8_t> &out) {
    EntropyLayout e;
    if (const char *problem = entropy_validate(p, len, e)) return problem;
    const CodecLayout &l = e.cwao;
    const size_t head = CODEC_HEADER_BYTES + 4u * (size_t)l.bits;
    out.assign((size_t)l.total_bytes, 0);
    memcpy(out.data(), p, head);
    const uint32_t magic = CODEC_MAGIC, version = CODEC_VERSION;
    memcpy(out.data(), &magic, 4);
    memcpy(out.data() + 4, &version, 4);
    std::vector<uint8_t> v;
    const int cb = l.colour_bits;
    for (int i = 0; i < e.nstreams; i++) {
        const EntropyStream &s = e.stream[i];
        if (const char *problem = entropy_read_payload(p + s.payload_offset, s, cb, v)) return problem;
        if (s.kind == ENTROPY_OCCUPANCY) {
            memcpy(out.data() + l.occupancy_offset + entropy_depth_offset(l, (int)s.which), v.data(), s.symbols);
        } else if (s.kind == ENTROPY_TILE) {
            memcpy(out.data() + l.tile_offset, v.data(), s.symbols);
        } else {
            for (uint64_t j = 0; j < s.symbols; j++) entropy_bits_put(out.data() + l.colour_offset, (3u * j + s.which) * (uint64_t)cb, cb, v[j]);
        }
    }
    return nullptr;
}

}  // namespace cwipc_amd
