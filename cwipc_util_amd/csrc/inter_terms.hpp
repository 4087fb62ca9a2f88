// inter_terms.hpp -- RULE P, inter-frame coding of the octree codec's packets (the rule in full: hip_ext.h; its numpy restatement:
// tests/inter_model.py).  A "cwap" packet is a key packet (a prefix in front of one complete "cwao" or "cwae" packet) or a delta
// packet, which stands for exactly one valid "cwao" packet P given the packet R before it: the leaves of R that stay (a bit each), the
// leaves that are new (an octree of their own), and per leaf of P the difference of its stored colour and tile to a leaf of R.  The
// streams are coded by RULE E's coder (entropy_terms.hpp), without its colour prediction.  Compiles for host and device:
// kernels_inter.hip, the codec_*.cpp files and the stand-alone host program of the tests (tests/abi/inter_host.cpp) include this one text.
// Every operation is rounded on its own: build with -ffp-contract=off.
#pragma once

#include "entropy_terms.hpp"

#include <vector>

namespace cwipc_amd {

constexpr uint32_t INTER_MAGIC = 0x70617763u;   // the bytes c w a p
constexpr uint32_t INTER_VERSION = 1u;
constexpr size_t INTER_PREFIX_BYTES = 32;
constexpr size_t INTER_HEADER_BYTES = 40;       // bytes 8 .. 48 of RULE C's header
constexpr uint32_t INTER_KEY = 0u, INTER_DELTA = 1u;
constexpr int INTER_MAX_GOP = 65535;
constexpr int INTER_MAX_STREAMS = 1 + CODEC_MAX_BITS + 4;

// ---------------------------------------------------------------------------
// the arithmetic (host and device)
// ---------------------------------------------------------------------------
// inter mode is on iff all three parameters ask for it; each alone is refused by the encoder's constructor
CW_CODEC_HD inline bool inter_exp_factor_ok(float exp_factor) { return exp_factor >= 1.0f && exp_factor <= 16.0f; }   // (false for a NaN)
CW_CODEC_HD inline bool inter_params_on(bool do_inter_frame, int gop_size, float exp_factor) {
    return do_inter_frame && gop_size >= 2 && gop_size <= INTER_MAX_GOP && inter_exp_factor_ok(exp_factor);
}

// The cube of a key frame from RULE C's cube of the frame: the side times exp_factor, the origin moved back by half the growth.
CW_CODEC_HD inline void inter_expand_cube(const float mn[3], double side, float exp_factor, float out_mn[3], double &out_side) {
    const double grown = side * (double)exp_factor;
    const double margin = (grown - side) * 0.5;
    for (int a = 0; a < 3; a++) out_mn[a] = (float)((double)mn[a] - margin) + 0.0f;   // (a zero is +0)
    out_side = grown;
}

// Is the frame with the float32 extremes lo, hi inside the cube (mn, side)?  Then every point's cell by RULE C is below 2^b unclamped
// or at the clamp with u == 1, as in the frame that made the cube.
CW_CODEC_HD inline bool inter_contained(const float lo[3], const float hi[3], const float mn[3], double side) {
    for (int a = 0; a < 3; a++) {
        if (!(lo[a] >= mn[a])) return false;
        if (!((((double)hi[a] - (double)mn[a]) / side) <= 1.0)) return false;
    }
    return true;
}

// The leaf of R that predicts a leaf of P with key k: the same leaf when R has it, otherwise R's predecessor in key order, R's first
// leaf when there is none.  `found`: R has the key.  keys ascending, n > 0.
CW_CODEC_HD inline uint32_t inter_upper_bound(const unsigned long long *keys, uint32_t n, unsigned long long k) {
    uint32_t lo = 0, hi = n;   // the number of keys <= k
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (keys[mid] <= k) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
CW_CODEC_HD inline uint32_t inter_predictor(const unsigned long long *keys, uint32_t n, unsigned long long k, bool &found) {
    const uint32_t ub = inter_upper_bound(keys, n, k);
    found = ub > 0u && keys[ub - 1u] == k;
    return ub > 0u ? ub - 1u : 0u;
}
CW_CODEC_HD inline uint32_t inter_colour_symbol(uint32_t vp, uint32_t vr, int cb) { return (vp - vr) & ((1u << cb) - 1u); }
CW_CODEC_HD inline uint32_t inter_colour_value(uint32_t vr, uint32_t symbol, int cb) { return (vr + symbol) & ((1u << cb) - 1u); }

// the state machine of an encoder: which kind the next frame has, and the counter after it
struct InterSequence {
    int gop_size = 2;
    int g = 0;
    bool have_reference = false;
    bool at_gop_boundary() const { return g == 0 || !have_reference; }
    // kind and gop_index of a frame; empty: P has no leaf; contained: the frame lies in the GOP's cube (looked at only when a delta is possible)
    uint32_t next(bool empty, bool contained, uint32_t &gop_index) {
        const bool key = g == 0 || !have_reference || empty || !contained;
        if (key) g = 0;
        gop_index = (uint32_t)g;
        have_reference = !empty;
        g = (g + 1) % gop_size;
        return key ? INTER_KEY : INTER_DELTA;
    }
};

// ---------------------------------------------------------------------------
// the packets (little endian)
// ---------------------------------------------------------------------------
struct InterReference {           // what a delta packet names of the frame before it, and what a decoder holds of it
    uint64_t timestamp = 0;
    uint32_t nleaves = 0;
    int bits = 0, colour_bits = 0;
    float mn[3] = {0, 0, 0};
    double side = 1.0;
};

struct InterLayout {
    uint32_t kind = 0, gop_index = 0;
    uint64_t ref_timestamp = 0;
    uint32_t ref_nleaves = 0;
    // key: the embedded packet
    bool embedded_entropy = false;
    // both: the header of the packet this one stands for (key: offsets and sizes of the embedded packet's "cwao" form; delta: nodes[]
    // and the offsets are not known before the delta has been applied and stay 0)
    CodecLayout cwao;
    // delta
    uint32_t nadded = 0;
    uint32_t nodes_added[CODEC_MAX_BITS] = {0};
    int nstreams = 0;
    EntropyStream stream[INTER_MAX_STREAMS];
    uint64_t directory_offset = 0;
    uint64_t total_bytes = 0;
};

inline void inter_write_prefix(uint8_t *p, uint32_t kind, uint32_t gop_index, uint64_t ref_timestamp, uint32_t ref_nleaves) {
    const uint32_t words[4] = {INTER_MAGIC, INTER_VERSION, kind, gop_index}, zero = 0;
    memcpy(p, words, 16);
    memcpy(p + 16, &ref_timestamp, 8);
    memcpy(p + 24, &ref_nleaves, 4);
    memcpy(p + 28, &zero, 4);
}

// where depth d's occupancy bytes start in the occupancy plane of the added leaves
inline uint64_t inter_depth_offset(const uint32_t nodes_added[], int d) {
    uint64_t at = 0;
    for (int i = 0; i < d; i++) at += i == 0 ? 1u : nodes_added[i - 1];
    return at;
}

// The streams of a delta in RULE P's order: keep, the added leaves' occupancy per depth, r, g, b, the tile; returns S.
inline int inter_streams(uint32_t ref_nleaves, uint32_t nleaves, int bits, int colour_bits, int tile_mode, uint32_t nadded, const uint32_t nodes_added[],
                         EntropyStream s[INTER_MAX_STREAMS]) {
    int n = 0;
    EntropyStream keep;
    keep.kind = ENTROPY_BYTES;
    keep.symbols = (uint32_t)(((uint64_t)ref_nleaves + 7u) / 8u);
    keep.raw_bytes = keep.symbols;
    s[n++] = keep;
    for (int d = 0; d < bits && nadded; d++) {
        EntropyStream e;
        e.kind = ENTROPY_OCCUPANCY;
        e.which = (uint32_t)d;
        e.symbols = d == 0 ? 1u : nodes_added[d - 1];
        e.children = nodes_added[d];
        e.raw_bytes = e.symbols;
        s[n++] = e;
    }
    for (int ch = 0; ch < 3; ch++) {
        EntropyStream e;
        e.kind = ENTROPY_BITS;
        e.which = (uint32_t)ch;
        e.symbols = nleaves;
        e.raw_bytes = ((uint64_t)nleaves * (uint64_t)colour_bits + 7u) / 8u;
        s[n++] = e;
    }
    if (tile_mode == 1) {
        EntropyStream e;
        e.kind = ENTROPY_BYTES;
        e.which = 1;
        e.symbols = nleaves;
        e.raw_bytes = nleaves;
        s[n++] = e;
    }
    for (int i = 0; i < n; i++) s[i].nblocks = entropy_block_count(s[i].symbols);
    return n;
}

// The container test of a "cwap" packet: host code, before anything is launched or allocated on the device.  `ref`: the reference a
// decoder holds (nullptr: the packet alone is looked at).  nullptr: right, `out` filled.  Nothing outside [p, p + len) is read.
inline const char *inter_validate(const uint8_t *p, size_t len, const InterReference *ref, InterLayout &out) {
    InterLayout e;
    if (p == nullptr) return "no packet";
    if (len < INTER_PREFIX_BYTES) return "truncated prefix";
    if (codec_read<uint32_t>(p) != INTER_MAGIC) return "wrong magic (not an inter-frame packet of this library's octree codec)";
    if (codec_read<uint32_t>(p + 4) != INTER_VERSION) return "unknown version";
    e.kind = codec_read<uint32_t>(p + 8);
    e.gop_index = codec_read<uint32_t>(p + 12);
    e.ref_timestamp = codec_read<uint64_t>(p + 16);
    e.ref_nleaves = codec_read<uint32_t>(p + 24);
    if (e.kind > INTER_DELTA) return "unknown packet kind";
    if (codec_read<uint32_t>(p + 28) != 0u) return "reserved word of the prefix is not 0";
    if (e.kind == INTER_KEY) {
        if (e.gop_index != 0u || e.ref_timestamp != 0u || e.ref_nleaves != 0u) return "key packet names a reference";
        const uint8_t *q = p + INTER_PREFIX_BYTES;
        const size_t qlen = len - INTER_PREFIX_BYTES;
        e.embedded_entropy = qlen >= 4 && codec_read<uint32_t>(q) == ENTROPY_MAGIC;
        if (e.embedded_entropy) {
            EntropyLayout el;
            if (const char *problem = entropy_validate(q, qlen, el)) return problem;
            e.cwao = el.cwao;
        } else {
            if (const char *problem = codec_validate(q, qlen, e.cwao)) return problem;
        }
        e.total_bytes = len;
        out = e;
        return nullptr;
    }
    if (e.gop_index < 1u || e.gop_index > (uint32_t)(INTER_MAX_GOP - 1)) return "gop_index of a delta packet outside 1..65534";
    if (e.ref_nleaves == 0u) return "delta packet against an empty reference";
    if (len < INTER_PREFIX_BYTES + INTER_HEADER_BYTES + 4u) return "truncated header";
    const uint8_t *h = p + INTER_PREFIX_BYTES - 8;   // h + i: byte i of RULE C's header, for i in 8 .. 48
    CodecLayout &l = e.cwao;
    l.timestamp = codec_read<uint64_t>(h + 8);
    l.nleaves = codec_read<uint32_t>(h + 16);
    l.bits = h[20];
    l.colour_bits = h[21];
    l.tile_mode = h[22];
    l.tile_value = h[23];
    if (l.bits < 1 || l.bits > CODEC_MAX_BITS) return "octree_bits outside 1..16";
    if (l.colour_bits < 4 || l.colour_bits > 8) return "colour bits outside 4..8";
    if (l.tile_mode > 1) return "unknown tile mode";
    if (l.tile_mode == 1 && l.tile_value != 0) return "tile value with a tile plane";
    if (codec_read<uint32_t>(h + 36) != 0u) return "reserved word is not 0";
    for (int a = 0; a < 3; a++) {
        l.mn[a] = codec_read<float>(h + 24 + 4 * a);
        if (!std::isfinite(l.mn[a])) return "cube origin is not finite";
    }
    l.side = codec_read<double>(h + 40);
    if (!std::isfinite(l.side) || !(l.side > 0.0)) return "cube side is not a positive finite number";
    if (l.nleaves == 0u) return "delta packet of an empty cloud";
    const size_t counts_at = INTER_PREFIX_BYTES + INTER_HEADER_BYTES;
    e.nadded = codec_read<uint32_t>(p + counts_at);
    if (e.nadded > l.nleaves) return "more added leaves than leaves";
    if ((uint64_t)l.nleaves - e.nadded > e.ref_nleaves) return "more kept leaves than the reference has";
    if (len < counts_at + 4u + 4u * (size_t)l.bits) return "truncated node counts";
    for (int d = 0; d < l.bits; d++) e.nodes_added[d] = codec_read<uint32_t>(p + counts_at + 4u + 4u * (size_t)d);
    if (e.nadded == 0u) {
        for (int d = 0; d < l.bits; d++) if (e.nodes_added[d] != 0u) return "node counts without added leaves";
    } else {
        if (e.nodes_added[l.bits - 1] != e.nadded) return "added leaf count differs from the deepest node count";
        if (e.nodes_added[0] < 1u || e.nodes_added[0] > 8u) return "first node count outside 1..8";
        for (int d = 0; d + 1 < l.bits; d++)
            if (e.nodes_added[d + 1] < e.nodes_added[d] || (uint64_t)e.nodes_added[d + 1] > 8u * (uint64_t)e.nodes_added[d]) return "node counts do not fit a tree";
    }
    e.directory_offset = counts_at + 4u + 4u * (uint64_t)l.bits;
    e.nstreams = inter_streams(e.ref_nleaves, l.nleaves, l.bits, l.colour_bits, l.tile_mode, e.nadded, e.nodes_added, e.stream);
    if (const char *problem = entropy_validate_streams(p, len, e.directory_offset, e.nstreams, e.stream, l.colour_bits, e.total_bytes)) return problem;
    if (ref != nullptr) {
        if (ref->nleaves == 0u) return "no reference is held (a key packet must come first)";
        if (ref->timestamp != e.ref_timestamp || ref->nleaves != e.ref_nleaves) return "the reference held is not the one the delta packet names";
        if (ref->bits != l.bits || ref->colour_bits != l.colour_bits || memcmp(ref->mn, l.mn, 12) != 0 || memcmp(&ref->side, &l.side, 8) != 0)
            return "the reference held has another cube or other bit counts";
    }
    out = e;
    return nullptr;
}

// ---------------------------------------------------------------------------
// whole packets on the host
// ---------------------------------------------------------------------------
// The leaves of a valid "cwao" packet: keys ascending, stored colours (3 a leaf), tiles (the tile value throughout without a plane).
struct InterLeaves {
    std::vector<unsigned long long> keys;
    std::vector<uint8_t> colour[3], tile;
};

inline void inter_leaves_of(const uint8_t *p, const CodecLayout &l, InterLeaves &out) {
    std::vector<unsigned long long> prefix(1, 0ull), next;
    const uint8_t *occ = p + l.occupancy_offset;
    for (int d = 0; d < l.bits && l.nleaves; d++) {
        next.clear();
        for (size_t i = 0; i < prefix.size(); i++)
            for (unsigned c = 0; c < 8; c++)
                if ((occ[i] >> c) & 1u) next.push_back((prefix[i] << 3) | c);
        occ += prefix.size();
        prefix.swap(next);
    }
    if (!l.nleaves) prefix.clear();
    out.keys.swap(prefix);
    EntropyStream s;
    s.kind = ENTROPY_COLOUR;
    s.symbols = l.nleaves;
    for (uint32_t ch = 0; ch < 3; ch++) {
        s.which = ch;
        entropy_stream_values(p, l, s, out.colour[ch]);
    }
    if (l.tile_mode == 1) out.tile.assign(p + l.tile_offset, p + l.tile_offset + l.nleaves);
    else out.tile.assign(l.nleaves, (uint8_t)l.tile_value);
}

// nodes[] and the occupancy bytes (no padding) of the tree whose leaves are `keys` (ascending, distinct, at least one)
inline void inter_tree_of(const std::vector<unsigned long long> &keys, int bits, uint32_t nodes[CODEC_MAX_BITS], std::vector<uint8_t> &occupancy) {
    occupancy.clear();
    for (int d = 0; d < bits; d++) {
        const int shift = 3 * (bits - 1 - d);
        uint32_t count = 0;
        unsigned long long last_child = ~0ull, last_parent = ~0ull;
        for (unsigned long long k : keys) {
            const unsigned long long child = k >> shift, parent = child >> 3;
            if (child == last_child) continue;
            if (parent != last_parent || count == 0) occupancy.push_back(0);
            occupancy.back() |= (uint8_t)(1u << (child & 7u));
            last_child = child;
            last_parent = parent;
            count++;
        }
        nodes[d] = count;
    }
}

// The "cwao" packet of leaves (at least one) under the header fields of `l` (timestamp, bits, colour_bits, tile_mode, tile_value, mn, side).
inline void inter_build_cwao(CodecLayout l, const InterLeaves &v, std::vector<uint8_t> &out) {
    std::vector<uint8_t> occupancy;
    l.nleaves = (uint32_t)v.keys.size();
    inter_tree_of(v.keys, l.bits, l.nodes, occupancy);
    codec_layout_sizes(l);
    out.assign((size_t)l.total_bytes, 0);
    codec_write_header(out.data(), l);
    memcpy(out.data() + l.occupancy_offset, occupancy.data(), occupancy.size());
    for (uint64_t j = 0; j < l.nleaves; j++)
        for (uint32_t ch = 0; ch < 3; ch++) entropy_bits_put(out.data() + l.colour_offset, (3u * j + ch) * (uint64_t)l.colour_bits, l.colour_bits, v.colour[ch][j]);
    if (l.tile_mode == 1) memcpy(out.data() + l.tile_offset, v.tile.data(), l.nleaves);
}

inline const char *inter_same_cube(const CodecLayout &r, const CodecLayout &p) {
    if (r.bits != p.bits || r.colour_bits != p.colour_bits) return "the two packets have different bit counts";
    if (memcmp(r.mn, p.mn, 12) != 0 || memcmp(&r.side, &p.side, 8) != 0) return "the two packets have different cubes";
    return nullptr;
}

// A key packet around a valid "cwao" or "cwae" packet.
inline void inter_key_packet(const uint8_t *embedded, size_t len, std::vector<uint8_t> &out) {
    out.assign(INTER_PREFIX_BYTES + len, 0);
    inter_write_prefix(out.data(), INTER_KEY, 0, 0, 0);
    memcpy(out.data() + INTER_PREFIX_BYTES, embedded, len);
}

// diff(P, R): the delta packet of the valid "cwao" packet P against the valid "cwao" packet R (both with leaves, in one cube).
inline const char *inter_pack(const uint8_t *r, size_t rlen, const uint8_t *p, size_t plen, uint32_t gop_index, std::vector<uint8_t> &out) {
    CodecLayout lr, lp;
    if (const char *problem = codec_validate(r, rlen, lr)) return problem;
    if (const char *problem = codec_validate(p, plen, lp)) return problem;
    if (lr.nleaves == 0u || lp.nleaves == 0u) return "a delta packet needs leaves in both packets";
    if (const char *problem = inter_same_cube(lr, lp)) return problem;
    if (gop_index < 1u || gop_index > (uint32_t)(INTER_MAX_GOP - 1)) return "gop_index of a delta packet outside 1..65534";
    InterLeaves R, P;
    inter_leaves_of(r, lr, R);
    inter_leaves_of(p, lp, P);
    const uint32_t nr = lr.nleaves, np = lp.nleaves;
    const int cb = lp.colour_bits;
    std::vector<uint8_t> values[INTER_MAX_STREAMS];
    std::vector<uint8_t> &keep = values[0];
    keep.assign(((size_t)nr + 7u) / 8u, 0);
    std::vector<unsigned long long> added;
    std::vector<uint8_t> res[4];
    for (int c = 0; c < 4; c++) res[c].resize(np);
    for (uint32_t j = 0; j < np; j++) {
        bool found = false;
        const uint32_t pred = inter_predictor(R.keys.data(), nr, P.keys[j], found);
        if (found) keep[pred >> 3] |= (uint8_t)(1u << (pred & 7u));
        else added.push_back(P.keys[j]);
        for (int ch = 0; ch < 3; ch++) res[ch][j] = (uint8_t)inter_colour_symbol(P.colour[ch][j], R.colour[ch][pred], cb);
        res[3][j] = (uint8_t)(P.tile[j] ^ R.tile[pred]);
    }
    uint32_t nodes_added[CODEC_MAX_BITS] = {0};
    std::vector<uint8_t> occupancy;
    if (!added.empty()) inter_tree_of(added, lp.bits, nodes_added, occupancy);
    EntropyStream streams[INTER_MAX_STREAMS];
    const int S = inter_streams(nr, np, lp.bits, cb, lp.tile_mode, (uint32_t)added.size(), nodes_added, streams);
    int at = 1;
    for (int d = 0; d < lp.bits && !added.empty(); d++, at++) {
        const uint64_t from = inter_depth_offset(nodes_added, d);
        values[at].assign(occupancy.begin() + (ptrdiff_t)from, occupancy.begin() + (ptrdiff_t)(from + streams[at].symbols));
    }
    for (int c = 0; c < 3 + lp.tile_mode; c++, at++) values[at].swap(res[c]);
    const size_t head = INTER_PREFIX_BYTES + INTER_HEADER_BYTES + 4u + 4u * (size_t)lp.bits;
    out.assign(head + 4u + 8u * (size_t)S, 0);
    inter_write_prefix(out.data(), INTER_DELTA, gop_index, lr.timestamp, nr);
    memcpy(out.data() + INTER_PREFIX_BYTES, p + 8, INTER_HEADER_BYTES);
    const uint32_t nadded = (uint32_t)added.size(), count = (uint32_t)S;
    memcpy(out.data() + INTER_PREFIX_BYTES + INTER_HEADER_BYTES, &nadded, 4);
    memcpy(out.data() + INTER_PREFIX_BYTES + INTER_HEADER_BYTES + 4, nodes_added, 4u * (size_t)lp.bits);
    memcpy(out.data() + head, &count, 4);
    std::vector<uint8_t> payload;
    for (int i = 0; i < S; i++) {
        entropy_make_payload(streams[i], values[i], cb, payload);
        const uint32_t entry[2] = {streams[i].mode, (uint32_t)payload.size()};
        memcpy(out.data() + head + 4u + 8u * (size_t)i, entry, 8);
        out.insert(out.end(), payload.begin(), payload.end());
    }
    return nullptr;
}

// apply(D, R): the "cwao" packet the "cwap" packet d stands for; a key packet's embedded packet verbatim (r may be nullptr then).
inline const char *inter_unpack(const uint8_t *r, size_t rlen, const uint8_t *d, size_t dlen, std::vector<uint8_t> &out) {
    InterLayout e;
    if (const char *problem = inter_validate(d, dlen, nullptr, e)) return problem;
    if (e.kind == INTER_KEY) {
        out.assign(d + INTER_PREFIX_BYTES, d + dlen);
        return nullptr;
    }
    CodecLayout lr;
    if (const char *problem = codec_validate(r, rlen, lr)) return problem;
    InterReference ref;
    ref.timestamp = lr.timestamp;
    ref.nleaves = lr.nleaves;
    ref.bits = lr.bits;
    ref.colour_bits = lr.colour_bits;
    memcpy(ref.mn, lr.mn, 12);
    ref.side = lr.side;
    if (const char *problem = inter_validate(d, dlen, &ref, e)) return problem;
    const CodecLayout &l = e.cwao;
    const uint32_t nr = lr.nleaves, np = l.nleaves;
    const int cb = l.colour_bits;
    InterLeaves R, P;
    inter_leaves_of(r, lr, R);
    std::vector<uint8_t> values[INTER_MAX_STREAMS];
    for (int i = 0; i < e.nstreams; i++)
        if (const char *problem = entropy_read_payload(d + e.stream[i].payload_offset, e.stream[i], cb, values[i])) return problem;
    const std::vector<uint8_t> &keep = values[0];
    if ((nr & 7u) && (keep[nr >> 3] >> (nr & 7u))) return "padding bits of the kept leaves are not 0";
    uint64_t kept = 0;
    for (uint8_t b : keep) kept += (uint64_t)__builtin_popcount(b);
    if (kept + e.nadded != np) return "kept and added leaves differ from the leaf count";
    // the added leaves: their tree, depth by depth, as RULE C's decoder walks it
    std::vector<unsigned long long> added(e.nadded ? 1 : 0, 0ull), next;
    for (int depth = 0; depth < l.bits && e.nadded; depth++) {
        const std::vector<uint8_t> &occ = values[1 + depth];
        next.clear();
        for (size_t i = 0; i < added.size(); i++)
            for (unsigned c = 0; c < 8; c++)
                if ((occ[i] >> c) & 1u) next.push_back((added[i] << 3) | c);
        added.swap(next);
    }
    // the merge of the kept leaves of R and the added ones
    P.keys.reserve(np);
    size_t a = 0;
    for (uint32_t i = 0; i < nr; i++) {
        while (a < added.size() && added[a] < R.keys[i]) P.keys.push_back(added[a++]);
        if (a < added.size() && added[a] == R.keys[i]) return "an added leaf is a leaf of the reference";
        if ((keep[i >> 3] >> (i & 7u)) & 1u) P.keys.push_back(R.keys[i]);
    }
    while (a < added.size()) P.keys.push_back(added[a++]);
    const int first_colour = 1 + (e.nadded ? l.bits : 0);
    for (int ch = 0; ch < 3; ch++) P.colour[ch].resize(np);
    P.tile.resize(np);
    for (uint32_t j = 0; j < np; j++) {
        bool found = false;
        const uint32_t pred = inter_predictor(R.keys.data(), nr, P.keys[j], found);
        for (int ch = 0; ch < 3; ch++) P.colour[ch][j] = (uint8_t)inter_colour_value(R.colour[ch][pred], values[first_colour + ch][j], cb);
        P.tile[j] = l.tile_mode == 1 ? (uint8_t)(R.tile[pred] ^ values[first_colour + 3][j]) : (uint8_t)l.tile_value;
    }
    inter_build_cwao(l, P, out);
    return nullptr;
}

}  // namespace cwipc_amd
