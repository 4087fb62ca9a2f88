// codec_stage.hpp -- the octree codec's host staging, stated once: the plain structs the codec's kernels are handed, and the
// arithmetic that fills them (which stream goes where, how a device block is carved, what a status word means).  Free of HIP: it
// compiles with a plain host C++ compiler, so the stand-alone host program of the tests (tests/abi/codec_stage_host.cpp) checks every
// carve for bounds and overlap without a GPU.  internal.hpp includes it; codec_encode.cpp and codec_decode.cpp are its callers.
#pragma once

#include <cstdint>

#include "entropy_terms.hpp"
#include "inter_terms.hpp"
#include "transform_terms.hpp"

namespace cwipc_amd {

inline size_t stage_round256(size_t n) { return (n + 255) & ~(size_t)255; }

namespace k {

// ---- kernels_codec.hip ----
struct CodecLeafSum {
    unsigned long long r, g, b;
    uint32_t count, tile;
};
// One packet's body on the device, zeroed: occupancy (words; occupancy_bytes of them count), colours (colour_words words), the tile
// plane (nleaves bytes), tile_stats (2 words); and the leaf sums (nleaves, zeroed).  depth_offset[L]: the first occupancy byte of depth L.
struct CodecEmit {
    int bits;
    uint32_t nleaves;
    uint64_t depth_offset[16];
    uint64_t occupancy_bytes, colour_words;
    uint32_t *occupancy, *colours, *tile_stats;
    uint8_t *tiles;
    CodecLeafSum *sums;
};
struct CodecDecode {
    int bits, colour_bits, tile_value;
    uint32_t nleaves;
    uint32_t nodes[16];
    float mn[3];
    double cell;
    uint64_t colour_words;
    const uint32_t *colours;   // device, 4-byte aligned
    const uint8_t *tiles;      // device, or nullptr: tile_value
};

// ---- kernels_entropy.hip ----
constexpr int ENTROPY_STREAMS = 21;                      // RULE E: octree_bits + 3 + 1 at the most; RULE P: one more (keep)
constexpr size_t ENTROPY_SLOT_BYTES = 256 + 2 * 4096;    // a block's states and the most words it can emit
// The streams of one packet, in RULE E's order; block b of stream i is the global block first_block[i] + b.
struct EntropyStreams {
    int nstreams, colour_bits;
    uint32_t nleaves, total_blocks;
    uint32_t kind[ENTROPY_STREAMS], which[ENTROPY_STREAMS], symbols[ENTROPY_STREAMS], first_block[ENTROPY_STREAMS];
    uint32_t plane_offset[ENTROPY_STREAMS];   // occupancy: where the depth starts in the occupancy plane; ENTROPY_BYTES / _BITS: in `planes`
    uint32_t raw_padded[ENTROPY_STREAMS];     // the raw payload with its padding
};
// Encode: the body that codec_emit made (the tile stream is listed last and leaves when tile_stats says the tiles are uniform) -> `out`,
// zeroed by the caller, from the word S on.  report (device, 4 words): the bytes of `out` that count, S, and the two tile words.
struct EntropyEncode {
    EntropyStreams st;
    const uint8_t *planes;     // the byte planes of ENTROPY_BYTES / ENTROPY_BITS streams (RULE P), or nullptr
    const uint8_t *occupancy, *tiles;
    const uint32_t *colours, *tile_stats;
    uint64_t colour_words;
    uint32_t *hist;            // nstreams x 256, zeroed by the caller
    uint16_t *freq;            // nstreams x 256
    uint32_t *block_words, *block_bytes, *block_offset;   // total_blocks each
    uint8_t *slots;            // total_blocks x ENTROPY_SLOT_BYTES: states, then the words at the END of the slot in decoder order
    uint32_t *plan;            // nstreams x (mode, payload offset in `out`, payload bytes)
    uint32_t *report;
    uint8_t *out;
    uint64_t out_capacity;
};
// Decode: `in` is the packet from the word S on; per global block its offset in `in` and its size (coded streams; 0, 0 otherwise).
// The streams go to the body the octree decoder reads: occupancy bytes, the bit-packed colour plane (through `channels`, 3 x nleaves
// bytes), the tile plane.  status (pinned): tag << 32 | 1 a block is not intact | 2 an occupancy byte is 0 | 4 occupancy bits differ.
struct EntropyDecode {
    EntropyStreams st;
    uint32_t mode[ENTROPY_STREAMS], payload_offset[ENTROPY_STREAMS], payload_bytes[ENTROPY_STREAMS], children[ENTROPY_STREAMS];
    const uint8_t *in;
    const uint32_t *block_at;   // 2 x total_blocks: offset, bytes
    uint8_t *planes;            // where ENTROPY_BYTES / ENTROPY_BITS streams go (RULE P), or nullptr
    uint8_t *occupancy, *tiles, *channels;
    uint32_t *colours;          // nullptr: no colour plane is packed (RULE P's streams)
    uint64_t colour_words;
    uint32_t *flags;            // 1 + nstreams words, zeroed by the caller
};

// ---- kernels_transform.hip ----
// One packet's tree with the nodes numbered across depths (transform_terms.hpp): inner node i is occupancy byte i, the leaves are
// the numbers inner .. inner + nleaves - 1.  Depth L's parents are depth_begin[L] .. + depth_count[L].
struct TransformTree {
    int bits;
    uint32_t nleaves, inner;
    uint32_t depth_begin[16], depth_count[16];
    uint32_t q16[3], leaf_step[3];   // per channel: the scale, and the step of a butterfly of two leaves
    const uint8_t *occupancy;        // inner bytes
    uint32_t *first, *weight;        // inner words each: an inner node's first child, and the leaves beneath it
    int32_t *value;                  // 3 planes of inner + nleaves
    uint32_t *zz;                    // 3 planes of nleaves - 1: the zigzag values in coefficient order
    uint32_t *scan;                  // transform_scan_words() words
};

}  // namespace k

// ---- the stream table ----
// The streams s[0 .. n) as the entropy stage's kernels are handed them: kind, which, symbols, the blocks' numbering, the padded raw
// sizes and, by plane_offset(const EntropyStream &), where each stream's bytes lie on the device.  Returns the most bytes the streams
// take from the word S on (4 + 8 n + the padded raw sizes: a stream never takes more than its raw payload), or 0: more streams than
// the kernels' tables hold, nothing is to be launched.  st.colour_bits and st.nleaves are the caller's.
constexpr const char *STAGE_TOO_MANY_STREAMS = "more streams than the entropy stage's tables hold";
template <typename Rule>
inline size_t stage_streams(const EntropyStream *s, int n, Rule &&plane_offset, k::EntropyStreams &st) {
    if (n < 0 || n > k::ENTROPY_STREAMS) return 0;
    st.nstreams = n;
    st.total_blocks = 0;
    size_t capacity = 4 + 8u * (size_t)n;
    for (int i = 0; i < n; i++) {
        st.kind[i] = s[i].kind;
        st.which[i] = s[i].which;
        st.symbols[i] = s[i].symbols;
        st.first_block[i] = st.total_blocks;
        st.total_blocks += s[i].nblocks;
        st.plane_offset[i] = (uint32_t)plane_offset(s[i]);
        st.raw_padded[i] = (uint32_t)codec_pad4(s[i].raw_bytes);
        capacity += st.raw_padded[i];
    }
    return capacity;
}

// The three rules for plane_offset, one for the encoder and the decoder of each form.  RULE E: occupancy by depth in the body.
inline uint64_t stage_offset_rule_e(const CodecLayout &l, const EntropyStream &s) {
    return s.kind == ENTROPY_OCCUPANCY ? entropy_depth_offset(l, (int)s.which) : 0u;
}
// RULE T: as RULE E; channel ch's tokens are plane ch of nleaves - 1 bytes in `planes`.
inline uint64_t stage_offset_rule_t(const CodecLayout &l, const EntropyStream &s) {
    const uint64_t ncoef = l.nleaves ? (uint64_t)l.nleaves - 1u : 0u;
    return s.kind == ENTROPY_BYTES ? (uint64_t)s.which * ncoef : stage_offset_rule_e(l, s);
}
// RULE P: the added leaves' occupancy by depth; in `planes` keep at 0 and, from res_offset on, r, g, b and tile residuals of nleaves bytes.
inline uint64_t stage_offset_rule_p(const uint32_t nodes_added[], uint64_t res_offset, uint64_t nleaves, const EntropyStream &s) {
    return s.kind == ENTROPY_OCCUPANCY ? inter_depth_offset(nodes_added, (int)s.which)
           : s.kind == ENTROPY_BITS    ? res_offset + (uint64_t)s.which * nleaves
           : s.which == 1u             ? res_offset + 3 * nleaves
                                       : 0u;
}

// The decoder's four arrays behind stage_streams(): what the directory says of each stream (payload offsets from the word S on) and
// the bits an occupancy stream's bytes must hold, which every *_streams() list has left in `children`.
inline void stage_decode_streams(const EntropyStream *s, int n, uint64_t directory_offset, k::EntropyDecode &d) {
    for (int i = 0; i < n; i++) {
        d.mode[i] = s[i].mode;
        d.payload_offset[i] = (uint32_t)(s[i].payload_offset - directory_offset);
        d.payload_bytes[i] = (uint32_t)s[i].payload_bytes;
        d.children[i] = s[i].children;
    }
}

// RULE T: the escape streams do not go through the entropy stage.  The others of all[0 .. n) in their order into out; returns their number.
inline int stage_without_escapes(const EntropyStream *all, int n, EntropyStream *out) {
    int m = 0;
    for (int i = 0; i < n; i++)
        if (all[i].kind != TRANSFORM_ESCAPE) out[m++] = all[i];
    return m;
}

// The block table of a coded packet (2 x st.total_blocks words): per global block its offset from the word S on and its size; a
// coded stream's blocks lie behind its frequency table and its size words.  (0, 0) for the blocks of raw streams.
// (The container test has held the sizes to the payload.)
inline void stage_block_table(const EntropyStream *s, const k::EntropyStreams &st, const uint8_t *packet, uint64_t directory_offset, uint32_t *table) {
    memset(table, 0, 8u * (size_t)st.total_blocks);
    for (int i = 0; i < st.nstreams; i++) {
        if (s[i].mode != 1u) continue;
        uint32_t at = (uint32_t)(s[i].payload_offset - directory_offset) + ENTROPY_TABLE_BYTES + 4u * s[i].nblocks;
        for (uint32_t b = 0; b < s[i].nblocks; b++) {
            const uint32_t size = codec_read<uint32_t>(packet + s[i].payload_offset + ENTROPY_TABLE_BYTES + 4u * (size_t)b);
            table[2 * (st.first_block[i] + b)] = at;
            table[2 * (st.first_block[i] + b) + 1] = size;
            at += size;
        }
    }
}

// ---- device blocks ----
// The entropy encoder's work block for en.st: the size and the carve in one place.  Returns the bytes of the block; with `base` (the
// block, 256-aligned) the pointers of `en` are set into it.  Words first, the u16 table behind them, the slots on a 256-byte line.
inline size_t stage_encode_work(k::EntropyEncode &en, uint8_t *base) {
    const size_t S = (size_t)en.st.nstreams, nb = en.st.total_blocks;
    const size_t hist_at = 0, words_at = hist_at + S * 1024, bytes_at = words_at + nb * 4, offset_at = bytes_at + nb * 4, plan_at = offset_at + nb * 4,
                 report_at = plan_at + S * 12, freq_at = report_at + 16, slots_at = stage_round256(freq_at + S * 512);
    if (base) {
        en.hist = (uint32_t *)(base + hist_at);
        en.block_words = (uint32_t *)(base + words_at);
        en.block_bytes = (uint32_t *)(base + bytes_at);
        en.block_offset = (uint32_t *)(base + offset_at);
        en.plan = (uint32_t *)(base + plan_at);
        en.report = (uint32_t *)(base + report_at);
        en.freq = (uint16_t *)(base + freq_at);
        en.slots = base + slots_at;
    }
    return slots_at + nb * k::ENTROPY_SLOT_BYTES;
}

// RULE T's planes in one block: first, weight, the values, the zigzag values, the scans' words (scan_words of them) and the tokens,
// which encoder and decoder share; the encoder's escapes (3 planes of escape_stride u16) and its four report words behind them.
// From t.inner and t.nleaves; with `base` (the block) the tree's pointers are set into it.
struct StageTreePlanes {
    size_t tokens, escapes, report, bytes;
    uint32_t escape_stride;   // u16 values a channel: every coefficient, and the padding
};
inline StageTreePlanes stage_tree_planes(k::TransformTree &t, uint8_t *base, size_t scan_words, bool encoder) {
    const size_t inner = t.inner, n = t.nleaves, ncoef = n ? n - 1 : 0;
    const size_t weight_at = stage_round256(4 * inner), value_at = weight_at + stage_round256(4 * inner), zz_at = value_at + stage_round256(12 * (inner + n)),
                 scan_at = zz_at + stage_round256(12 * ncoef + 4);
    StageTreePlanes p{};
    p.escape_stride = (uint32_t)((n + 1u) & ~(size_t)1);
    p.tokens = scan_at + stage_round256(4 * scan_words);
    p.bytes = p.tokens + stage_round256(3 * ncoef + 4);
    if (encoder) {
        p.escapes = p.bytes;
        p.report = p.escapes + stage_round256(6 * (size_t)p.escape_stride);
        p.bytes = p.report + 256;
    }
    if (base) {
        t.first = (uint32_t *)base;
        t.weight = (uint32_t *)(base + weight_at);
        t.value = (int32_t *)(base + value_at);
        t.zz = (uint32_t *)(base + zz_at);
        t.scan = (uint32_t *)(base + scan_at);
    }
    return p;
}

// ---- small terms ----
// What the octree decoder's kernels are told of the packet of `l`, handing out `bits` octree bits at `colour_bits` in cells of `cell`;
// the colour and tile planes are the caller's to point at.
inline k::CodecDecode stage_decode_terms(const CodecLayout &l, int bits, int colour_bits, double cell) {
    k::CodecDecode d{};
    d.bits = bits;
    d.colour_bits = colour_bits;
    d.tile_value = l.tile_value;
    d.nleaves = l.nleaves;
    for (int i = 0; i < l.bits; i++) d.nodes[i] = l.nodes[i];
    for (int a = 0; a < 3; a++) d.mn[a] = l.mn[a];
    d.cell = cell;
    d.colour_words = codec_pad4(l.colour_bytes) / 4;
    return d;
}

// the two tile words the leaf kernel leaves: no bit set in both says one tile value throughout (the first word's low byte), else a plane
inline void stage_tile_words(uint32_t w0, uint32_t w1, int &tile_mode, int &tile_value) {
    const bool uniform = (w0 & w1) == 0u;
    tile_mode = uniform ? 0 : 1;
    tile_value = uniform ? (int)(w0 & 255u) : 0;
}

// why a decoder refuses a packet whose status word (the entropy stage's | RULE P's checks) is not 0; nullptr: it is 0
inline const char *stage_refusal(uint32_t status) {
    return status & 1u    ? "entropy-coded block is not intact"
           : status & 2u  ? "occupancy byte is 0"
           : status & 4u  ? "occupancy bits differ from the node count"
           : status & 16u ? "padding bits of the kept leaves are not 0"
           : status & 32u ? "kept and added leaves differ from the leaf count"
           : status & 8u  ? "an added leaf is a leaf of the reference"
                          : nullptr;
}

}  // namespace cwipc_amd
