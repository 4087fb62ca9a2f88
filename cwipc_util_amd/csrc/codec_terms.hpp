// codec_terms.hpp -- the arithmetic and the packet layout of RULE C, the octree codec (the rule in full: hip_ext.h; its numpy
// restatement: tests/codec_model.py).  Compiles for host and device: kernels_codec.hip, the codec_*.cpp files and the stand-alone host program
// of the tests (tests/abi/codec_packet_host.cpp) include this one text.  Every operation is rounded on its own: build with
// -ffp-contract=off.  The packets are this library's own (magic "cwao"); they are NOT cwipc_codec's bitstream.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define CW_CODEC_HD __host__ __device__
#else
#define CW_CODEC_HD
#endif

namespace cwipc_amd {

constexpr uint32_t CODEC_MAGIC = 0x6f617763u;   // the bytes c w a o
constexpr uint32_t CODEC_VERSION = 1u;
constexpr int CODEC_MAX_BITS = 16;
constexpr size_t CODEC_HEADER_BYTES = 48;       // in front of nodes[]

// jpeg_quality -> the colour shift s (8 - s bits are kept per channel)
CW_CODEC_HD inline int codec_colour_shift(int jpeg_quality) {
    return jpeg_quality >= 90 ? 0 : jpeg_quality >= 75 ? 1 : jpeg_quality >= 50 ? 2 : jpeg_quality >= 25 ? 3 : 4;
}
// a leaf's channel: the rounded mean of its points in integers, what the packet stores of it, and what comes back
CW_CODEC_HD inline uint32_t codec_leaf_mean(uint64_t sum, uint32_t count) { return (uint32_t)((sum + (uint64_t)(count / 2u)) / (uint64_t)count); }
CW_CODEC_HD inline uint32_t codec_colour_store(uint32_t m, int s) { return m >> s; }
CW_CODEC_HD inline uint32_t codec_colour_load(uint32_t v, int s) {
    const uint32_t d = (v << s) + ((1u << s) >> 1);
    return d > 255u ? 255u : d;
}

// The cube: min per axis as float32 (a zero is +0: min + 0.0f), side = the largest float64 extent, 1 where that is 0.
CW_CODEC_HD inline float codec_min_canonical(float mn) { return mn + 0.0f; }
CW_CODEC_HD inline double codec_side(const float mn[3], const float mx[3]) {
    double side = 0.0;
    for (int a = 0; a < 3; a++) {
        const double e = (double)mx[a] - (double)mn[a];
        if (e > side) side = e;
    }
    return side == 0.0 ? 1.0 : side;
}

// q_a = min(2^b - 1, (int) floor(u * 2^b)), u = fl64(fl64(p - min) / side); p >= min, both finite
CW_CODEC_HD inline uint32_t codec_cell(float p, float mn, double side, int bits) {
    const double u = ((double)p - (double)mn) / side;
    const double f = floor(u * (double)(1u << bits));
    const double top = (double)((1u << bits) - 1u);
    return f >= top ? (uint32_t)top : (uint32_t)f;
}

// bit i of v to bit 3 i (v < 2^16)
CW_CODEC_HD inline uint64_t codec_spread3(uint32_t v) {
    uint64_t x = v & 0xffffu;
    x = (x | (x << 16)) & 0x0000ff0000ffull;
    x = (x | (x << 8)) & 0x00f00f00f00full;
    x = (x | (x << 4)) & 0x0c30c30c30c3ull;
    x = (x | (x << 2)) & 0x249249249249ull;
    return x;
}
CW_CODEC_HD inline uint32_t codec_gather3(uint64_t x) {
    x &= 0x249249249249ull;
    x = (x | (x >> 2)) & 0x0c30c30c30c3ull;
    x = (x | (x >> 4)) & 0x00f00f00f00full;
    x = (x | (x >> 8)) & 0x0000ff0000ffull;
    x = (x | (x >> 16)) & 0xffffull;
    return (uint32_t)x;
}
// The 3b-bit key: most significant triple first, within a triple x, y, z with x most significant.
CW_CODEC_HD inline uint64_t codec_key(uint32_t qx, uint32_t qy, uint32_t qz) {
    return (codec_spread3(qx) << 2) | (codec_spread3(qy) << 1) | codec_spread3(qz);
}
CW_CODEC_HD inline void codec_unkey(uint64_t key, uint32_t q[3]) {
    q[0] = codec_gather3(key >> 2);
    q[1] = codec_gather3(key >> 1);
    q[2] = codec_gather3(key);
}

// decoding: the centre of the cell
CW_CODEC_HD inline double codec_cellsize(double side, int bits) { return side / (double)(1u << bits); }
CW_CODEC_HD inline float codec_position(float mn, uint32_t q, double cell) { return (float)((double)mn + (((double)q + 0.5) * cell)); }

// ---------------------------------------------------------------------------
// the packet (little endian)
// ---------------------------------------------------------------------------
struct CodecLayout {
    uint64_t timestamp = 0;
    uint32_t nleaves = 0;
    int bits = 0, colour_bits = 0, tile_mode = 0, tile_value = 0;
    float mn[3] = {0, 0, 0};
    double side = 1.0;
    uint32_t nodes[CODEC_MAX_BITS] = {0};
    uint64_t occupancy_offset = 0, occupancy_bytes = 0;   // bytes without the padding
    uint64_t colour_offset = 0, colour_bytes = 0;
    uint64_t tile_offset = 0, total_bytes = 0;
};

inline uint64_t codec_pad4(uint64_t n) { return (n + 3u) & ~(uint64_t)3u; }

// Fills the offsets and sizes from nleaves, bits, colour_bits, tile_mode and nodes[].
inline void codec_layout_sizes(CodecLayout &l) {
    l.occupancy_offset = CODEC_HEADER_BYTES + 4u * (uint64_t)l.bits;
    l.occupancy_bytes = 0;
    if (l.nleaves) {
        l.occupancy_bytes = 1;
        for (int d = 0; d + 1 < l.bits; d++) l.occupancy_bytes += l.nodes[d];
    }
    l.colour_offset = l.occupancy_offset + codec_pad4(l.occupancy_bytes);
    l.colour_bytes = ((uint64_t)l.nleaves * 3u * (uint64_t)l.colour_bits + 7u) / 8u;
    l.tile_offset = l.colour_offset + codec_pad4(l.colour_bytes);
    l.total_bytes = l.tile_offset + (l.tile_mode == 1 ? (uint64_t)l.nleaves : 0u);
}

template <typename T>
inline T codec_read(const uint8_t *p) {
    T v;
    memcpy(&v, p, sizeof(T));
    return v;
}

inline void codec_write_header(uint8_t *p, const CodecLayout &l) {
    memset(p, 0, CODEC_HEADER_BYTES + 4u * (size_t)l.bits);
    const uint32_t magic = CODEC_MAGIC, version = CODEC_VERSION;
    memcpy(p, &magic, 4);
    memcpy(p + 4, &version, 4);
    memcpy(p + 8, &l.timestamp, 8);
    memcpy(p + 16, &l.nleaves, 4);
    p[20] = (uint8_t)l.bits;
    p[21] = (uint8_t)l.colour_bits;
    p[22] = (uint8_t)l.tile_mode;
    p[23] = (uint8_t)l.tile_value;
    memcpy(p + 24, l.mn, 12);
    memcpy(p + 40, &l.side, 8);
    memcpy(p + CODEC_HEADER_BYTES, l.nodes, 4u * (size_t)l.bits);
}

// The header and nodes[] of a packet that starts with `magic`: ranges and the tree rule; the offsets and sizes of `l` are those of the
// "cwao" form.  nullptr: right, `l` filled.  The entropy-coded form (entropy_terms.hpp) carries the same bytes 8 .. 48 + 4 bits.
inline const char *codec_validate_header(const uint8_t *p, size_t len, uint32_t magic, CodecLayout &l) {
    if (p == nullptr) return "no packet";
    if (len < CODEC_HEADER_BYTES) return "truncated header";
    if (codec_read<uint32_t>(p) != magic) return "wrong magic (not a packet of this library's octree codec)";
    if (codec_read<uint32_t>(p + 4) != CODEC_VERSION) return "unknown version";
    l.timestamp = codec_read<uint64_t>(p + 8);
    l.nleaves = codec_read<uint32_t>(p + 16);
    l.bits = p[20];
    l.colour_bits = p[21];
    l.tile_mode = p[22];
    l.tile_value = p[23];
    if (l.bits < 1 || l.bits > CODEC_MAX_BITS) return "octree_bits outside 1..16";
    if (l.colour_bits < 4 || l.colour_bits > 8) return "colour bits outside 4..8";
    if (l.tile_mode > 1) return "unknown tile mode";
    if (l.tile_mode == 1 && l.tile_value != 0) return "tile value with a tile plane";
    if (codec_read<uint32_t>(p + 36) != 0u) return "reserved word is not 0";
    for (int a = 0; a < 3; a++) {
        l.mn[a] = codec_read<float>(p + 24 + 4 * a);
        if (!std::isfinite(l.mn[a])) return "cube origin is not finite";
    }
    l.side = codec_read<double>(p + 40);
    if (!std::isfinite(l.side) || !(l.side > 0.0)) return "cube side is not a positive finite number";
    if (len < CODEC_HEADER_BYTES + 4u * (size_t)l.bits) return "truncated node counts";
    for (int d = 0; d < l.bits; d++) l.nodes[d] = codec_read<uint32_t>(p + CODEC_HEADER_BYTES + 4 * d);
    if (l.nodes[l.bits - 1] != l.nleaves) return "leaf count differs from the deepest node count";
    if (l.nleaves == 0) {
        for (int d = 0; d < l.bits; d++) if (l.nodes[d] != 0) return "node counts of an empty cloud";
        if (l.tile_mode != 0 || l.tile_value != 0) return "tile fields of an empty cloud";
        const uint32_t zeros[3] = {codec_read<uint32_t>(p + 24), codec_read<uint32_t>(p + 28), codec_read<uint32_t>(p + 32)};
        if (zeros[0] || zeros[1] || zeros[2] || l.side != 1.0) return "cube of an empty cloud";
    } else {
        if (l.nodes[0] < 1 || l.nodes[0] > 8) return "first node count outside 1..8";
        for (int d = 0; d + 1 < l.bits; d++)
            if (l.nodes[d + 1] < l.nodes[d] || (uint64_t)l.nodes[d + 1] > 8u * (uint64_t)l.nodes[d]) return "node counts do not fit a tree";
    }
    codec_layout_sizes(l);
    return nullptr;
}

// One pass over the packet.  nullptr: valid, `out` filled; otherwise why not.  Nothing outside [p, p + len) is read.
inline const char *codec_validate(const uint8_t *p, size_t len, CodecLayout &out) {
    CodecLayout l;
    if (const char *problem = codec_validate_header(p, len, CODEC_MAGIC, l)) return problem;
    if ((uint64_t)len < l.total_bytes) return "truncated packet";
    if ((uint64_t)len > l.total_bytes) return "bytes behind the packet";
    // occupancy: depth d has 1, nodes[0], nodes[1] ... bytes, none 0, their bits as many as the next depth's nodes
    const uint8_t *occ = p + l.occupancy_offset;
    uint64_t at = 0;
    for (int d = 0; d < l.bits && l.nleaves; d++) {
        const uint64_t n = d == 0 ? 1u : l.nodes[d - 1];
        uint64_t children = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint8_t b = occ[at + i];
            if (b == 0) return "occupancy byte is 0";
            children += (uint64_t)__builtin_popcount(b);
        }
        if (children != l.nodes[d]) return "occupancy bits differ from the node count";
        at += n;
    }
    for (uint64_t i = l.occupancy_bytes; i < codec_pad4(l.occupancy_bytes); i++)
        if (occ[i] != 0) return "padding is not 0";
    const uint8_t *col = p + l.colour_offset;
    const uint64_t colour_bit_count = (uint64_t)l.nleaves * 3u * (uint64_t)l.colour_bits;
    if (colour_bit_count & 7u)
        if (col[l.colour_bytes - 1] >> (colour_bit_count & 7u)) return "padding is not 0";
    for (uint64_t i = l.colour_bytes; i < codec_pad4(l.colour_bytes); i++)
        if (col[i] != 0) return "padding is not 0";
    out = l;
    return nullptr;
}

}  // namespace cwipc_amd
