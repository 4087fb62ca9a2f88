// lod_terms.hpp -- the arithmetic of RULE L, level-of-detail cuts of octree packets (the rule in full: hip_ext.h; its numpy
// restatement: tests/lod_model.py).  Compiles for host and device: kernels_lod.hip, the codec_*.cpp files and the stand-alone host program of the
// tests (tests/abi/lod_host.cpp) include this one text.  Integers only.  The host half (lod_cut, lod_convert) is the twin of the
// kernels: it makes the packet L(P, t); the decoder's kernels make the cloud that decoding that packet gives.
#pragma once

#include "entropy_terms.hpp"
#include "inter_terms.hpp"
#include "transform_terms.hpp"

#include <vector>

namespace cwipc_amd {

// a new leaf's channel from the sum of its n >= 1 members' STORED values: the rounded mean in integers
CW_CODEC_HD inline uint32_t lod_mean(uint64_t sum, uint32_t n) { return (uint32_t)((sum + (uint64_t)(n / 2u)) / (uint64_t)n); }
// the key prefix of t triples of a key of b >= t triples: the new leaf a leaf lies under
CW_CODEC_HD inline uint64_t lod_prefix(uint64_t key, int b, int t) { return key >> (3 * (b - t)); }
// whether a leaf starts a run: the first leaf, or one whose prefix differs from its predecessor's (keys ascending)
CW_CODEC_HD inline bool lod_run_head(uint64_t before, uint64_t key, int b, int t, bool first) { return first || lod_prefix(before, b, t) != lod_prefix(key, b, t); }

// ---------------------------------------------------------------------------
// the packet function (host)
// ---------------------------------------------------------------------------
// RULE C's empty packet of t bits with P's timestamp and colour bits
inline void lod_empty(const CodecLayout &p, int t, std::vector<uint8_t> &out) {
    CodecLayout l;
    l.timestamp = p.timestamp;
    l.bits = t;
    l.colour_bits = p.colour_bits;
    codec_layout_sizes(l);
    out.assign((size_t)l.total_bytes, 0);
    codec_write_header(out.data(), l);
}

// L(P, t) of a "cwao" packet.  nullptr: done, `out` holds the packet; otherwise why not.
inline const char *lod_cut(const uint8_t *p, size_t len, int t, std::vector<uint8_t> &out) {
    CodecLayout l;
    if (const char *problem = codec_validate(p, len, l)) return problem;
    if (t < 1) return "octree bits of the cut below 1";
    if (t > l.bits) return "octree bits of the cut above the packet's";
    if (t == l.bits) { out.assign(p, p + len); return nullptr; }
    if (!l.nleaves) { lod_empty(l, t, out); return nullptr; }
    // the leaves under every node of depth t: from the deepest occupancy bytes up, a node's count is the sum of its children's
    const uint8_t *occ = p + l.occupancy_offset;
    std::vector<uint64_t> depth_at((size_t)l.bits + 1, 0);
    for (int d = 0; d < l.bits; d++) depth_at[(size_t)d + 1] = depth_at[(size_t)d] + (d == 0 ? 1u : l.nodes[d - 1]);
    std::vector<uint32_t> run(l.nodes[l.bits - 2]);
    for (size_t i = 0; i < run.size(); i++) run[i] = (uint32_t)__builtin_popcount(occ[depth_at[(size_t)l.bits - 1] + i]);
    for (int d = l.bits - 2; d >= t; d--) {
        const size_t n = l.nodes[d - 1];
        size_t child = 0;
        for (size_t i = 0; i < n; i++) {
            uint32_t sum = 0;
            for (int k = __builtin_popcount(occ[depth_at[(size_t)d] + i]); k > 0 && child < run.size(); k--) sum += run[child++];
            run[i] = sum;   // (i < child: a node has a child)
        }
        run.resize(n);
    }
    CodecLayout o;
    o.timestamp = l.timestamp;
    o.bits = t;
    o.colour_bits = l.colour_bits;
    o.nleaves = l.nodes[t - 1];
    for (int d = 0; d < t; d++) o.nodes[d] = l.nodes[d];
    for (int a = 0; a < 3; a++) o.mn[a] = l.mn[a];
    o.side = l.side;
    const size_t n = o.nleaves;
    if (run.size() != n) return "leaf runs differ from the node count";
    std::vector<uint8_t> tiles(n, 0);
    std::vector<uint32_t> stored(3 * n, 0);
    const uint8_t *col = p + l.colour_offset, *til = p + l.tile_offset;
    uint64_t at = 0;
    for (size_t j = 0; j < n; j++) {
        uint64_t sum[3] = {0, 0, 0};
        uint32_t tile = 0;
        if (run[j] < 1 || at + run[j] > l.nleaves) return "leaf runs differ from the leaf count";
        for (uint64_t i = at; i < at + run[j]; i++) {
            for (uint64_t ch = 0; ch < 3; ch++) sum[ch] += entropy_bits_at(col, l.colour_bytes, (3u * i + ch) * (uint64_t)l.colour_bits, l.colour_bits);
            tile |= l.tile_mode == 1 ? til[i] : (uint32_t)l.tile_value;
        }
        for (size_t ch = 0; ch < 3; ch++) stored[3 * j + ch] = lod_mean(sum[ch], run[j]);
        tiles[j] = (uint8_t)tile;
        at += run[j];
    }
    if (at != l.nleaves) return "leaf runs differ from the leaf count";
    bool uniform = true;
    for (size_t j = 1; j < n; j++) uniform = uniform && tiles[j] == tiles[0];
    o.tile_mode = uniform ? 0 : 1;
    o.tile_value = uniform ? tiles[0] : 0;
    codec_layout_sizes(o);
    out.assign((size_t)o.total_bytes, 0);
    codec_write_header(out.data(), o);
    memcpy(out.data() + o.occupancy_offset, occ, (size_t)o.occupancy_bytes);
    for (size_t v = 0; v < 3 * n; v++) entropy_bits_put(out.data() + o.colour_offset, (uint64_t)v * (uint64_t)o.colour_bits, o.colour_bits, stored[v]);
    if (o.tile_mode == 1) memcpy(out.data() + o.tile_offset, tiles.data(), n);
    return nullptr;
}

// The packet function: "cwao" -> L(P, t); "cwae" -> entropy_pack(L(entropy_unpack(Q), t)); the other forms are refused.
inline const char *lod_convert(const uint8_t *p, size_t len, int t, std::vector<uint8_t> &out) {
    if (p == nullptr) return "no packet";
    if (len < 4) return "truncated header";
    const uint32_t magic = codec_read<uint32_t>(p);
    if (magic == TRANSFORM_MAGIC) return "a \"cwat\" packet is not cut in one call: compose with cwipc_hip_codec_transform_unpack";
    if (magic == INTER_MAGIC) return "a \"cwap\" packet is not cut in one call: compose with cwipc_hip_codec_inter_unpack";
    if (magic != ENTROPY_MAGIC) return lod_cut(p, len, t, out);
    std::vector<uint8_t> plain, cut;
    if (const char *problem = entropy_unpack(p, len, plain)) return problem;
    if (const char *problem = lod_cut(plain.data(), plain.size(), t, cut)) return problem;
    return entropy_pack(cut.data(), cut.size(), out);
}

}  // namespace cwipc_amd
