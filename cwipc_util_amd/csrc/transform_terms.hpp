// transform_terms.hpp -- RULE T, transform colour coding of the octree codec's packets (the rule in full: hip_ext.h; its numpy
// restatement: tests/transform_model.py).  A "cwat" packet stands for exactly one valid "cwao" packet with 8 colour bits (RULE C,
// codec_terms.hpp): the same header, occupancy and tiles, and the colours that the integer transform gives back.  The transform is a
// weighted Haar lifting up the octree (RAHT with integer steps), exactly invertible at Q16 == 16; its quantised coefficients travel as
// byte tokens and u16 escapes through RULE E's container (entropy_terms.hpp).  Compiles for host and device: kernels_transform.hip,
// the codec_*.cpp files and the stand-alone host program of the tests (tests/abi/transform_host.cpp) include this one text.  Integers only.
//
// Nodes are numbered across depths: the root is 0, the nodes of a depth follow those of the depth above in ascending prefix order, so
// an inner node's number is the index of its occupancy byte, its children are 1 + (the occupancy bits in front of that byte) onwards,
// and the leaves are the last nleaves numbers.  The first coefficient of inner node i with first child s sits at s - i - 1.
#pragma once

#include "entropy_terms.hpp"

namespace cwipc_amd {

constexpr uint32_t TRANSFORM_MAGIC = 0x74617763u;   // the bytes c w a t
constexpr uint32_t TRANSFORM_VERSION = 1u;
constexpr uint32_t TRANSFORM_Q16_MIN = 16u, TRANSFORM_Q16_MAX = 1024u;
constexpr uint32_t TRANSFORM_FIXED_BYTES = 20u;     // u16 Q16, i16 dc[3], u32 nescapes[3]
constexpr uint32_t TRANSFORM_ESCAPE = 5u;           // a stream kind next to EntropyKind's: u16 values, always raw
constexpr int TRANSFORM_MAX_STREAMS = CODEC_MAX_BITS + 7;

// ---------------------------------------------------------------------------
// the arithmetic (host and device)
// ---------------------------------------------------------------------------
CW_CODEC_HD inline uint32_t transform_q16(int jpeg_quality) {
    const int q = jpeg_quality < 1 ? 1 : jpeg_quality;
    const int sc = q < 50 ? 5000 / q : 200 - 2 * q;
    const int v = 16 + (12 * sc) / 10;
    return (uint32_t)(v > 1024 ? 1024 : v);
}
// the scale of channel ch (0 Y, 1 Co, 2 Cg)
CW_CODEC_HD inline uint32_t transform_channel_q16(uint32_t q16, int ch) {
    if (ch == 0 || q16 == TRANSFORM_Q16_MIN) return q16;
    return 2u * q16 > TRANSFORM_Q16_MAX ? TRANSFORM_Q16_MAX : 2u * q16;
}

// reversible YCoCg-R; the shifts are arithmetic
CW_CODEC_HD inline void transform_to_ycocg(int32_t r, int32_t g, int32_t b, int32_t v[3]) {
    const int32_t co = r - b, t = b + (co >> 1), cg = g - t;
    v[0] = t + (cg >> 1);
    v[1] = co;
    v[2] = cg;
}
CW_CODEC_HD inline uint32_t transform_clamp255(int32_t v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }
// -> r | g << 8 | b << 16, every channel clamped
CW_CODEC_HD inline uint32_t transform_to_rgb(int32_t y, int32_t co, int32_t cg) {
    const int32_t t = y - (cg >> 1), g = cg + t, b = t - (co >> 1), r = b + co;
    return transform_clamp255(r) | (transform_clamp255(g) << 8) | (transform_clamp255(b) << 16);
}

// the exact floor of the square root
CW_CODEC_HD inline uint64_t transform_isqrt(uint64_t v) {
    if (v <= 0xffffffffull) {   // (a step's t is below 2^22: the same steps in 32 bits)
        uint32_t u = (uint32_t)v, r = 0, bit = 1u << 30;
        while (bit > u) bit >>= 2;
        for (; bit; bit >>= 2) {
            if (u >= r + bit) {
                u -= r + bit;
                r = (r >> 1) + bit;
            } else {
                r >>= 1;
            }
        }
        return r;
    }
    uint64_t r = 0, bit = 1ull << 62;
    while (bit > v) bit >>= 2;
    for (; bit; bit >>= 2) {
        if (v >= r + bit) {
            v -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
    }
    return r;
}

// floor(n / d) towards minus infinity, d > 0
CW_CODEC_HD inline int64_t transform_floor_div(int64_t n, int64_t d) {
    const int64_t q = n / d;
    return (n % d) < 0 ? q - 1 : q;
}

// the quantiser step of a butterfly of the weights w1, w2 (both above 0, their sum at most 2^32) at the channel scale q16
CW_CODEC_HD inline uint32_t transform_step(uint32_t q16, uint32_t w1, uint32_t w2) {
    const uint64_t t = ((uint64_t)q16 * q16 * ((uint64_t)w1 + w2)) / ((uint64_t)w1 * w2);
    const uint64_t s = (transform_isqrt(t) + 8u) >> 4;
    return s < 1u ? 1u : (uint32_t)s;
}

// the butterfly: (a, w1), (b, w2) -> the merged value l and the coefficient d; and back
CW_CODEC_HD inline int64_t transform_lift(int64_t d, uint32_t w1, uint32_t w2) {
    if (w1 == 1u && w2 == 1u) return (d + 1) >> 1;   // two leaves, nearly every butterfly of the deepest level: floor((d + 1) / 2)
    const int64_t W = (int64_t)w1 + (int64_t)w2;
    return transform_floor_div((int64_t)w2 * d + (W >> 1), W);
}
CW_CODEC_HD inline int64_t transform_quantise(int64_t d, uint32_t step) {
    const uint64_t a = (uint64_t)(d < 0 ? -d : d) + (uint64_t)(step / 2u);
    const int64_t m = a <= 0xffffffffull ? (int64_t)((uint32_t)a / step) : (int64_t)(a / step);   // (the encoder's d is a few hundred: a 32-bit division)
    return d < 0 ? -m : m;
}
CW_CODEC_HD inline uint32_t transform_zigzag(int64_t c) { return (uint32_t)(c >= 0 ? 2 * c : -2 * c - 1); }
CW_CODEC_HD inline int64_t transform_unzigzag(uint32_t zz) { return (zz & 1u) ? -(int64_t)((zz + 1u) >> 1) : (int64_t)(zz >> 1); }

// The seven places a parent's butterflies can take, in coefficient order: 0 the x butterfly, 1 and 2 the y butterflies (low half
// first), 3 .. 6 the z butterflies of the children (0,1), (2,3), (4,5), (6,7).  w[c]: the weight of child c = 4x + 2y + z, 0 where
// there is none.  Place k holds a butterfly iff w1[k] and w2[k] are both above 0.  Returns the parent's weight.
CW_CODEC_HD inline uint32_t transform_places(const uint32_t w[8], uint32_t w1[7], uint32_t w2[7]) {
    for (int k = 0; k < 4; k++) {
        w1[3 + k] = w[2 * k];
        w2[3 + k] = w[2 * k + 1];
    }
    w1[1] = w[0] + w[1];
    w2[1] = w[2] + w[3];
    w1[2] = w[4] + w[5];
    w2[2] = w[6] + w[7];
    w1[0] = w1[1] + w2[1];
    w2[0] = w1[2] + w2[2];
    return w1[0] + w2[0];
}

CW_CODEC_HD inline int64_t transform_pair(int64_t a, uint32_t w1, int64_t b, uint32_t w2, int64_t &d) {
    d = 0;
    if (!w2) return a;
    if (!w1) return b;
    d = b - a;
    return a + transform_lift(d, w1, w2);
}
CW_CODEC_HD inline void transform_unpair(int64_t l, uint32_t w1, uint32_t w2, int64_t d, int64_t &a, int64_t &b) {
    a = b = l;   // (one side empty: the other is the value passed through)
    if (!w1 || !w2) return;
    a = l - transform_lift(d, w1, w2);
    b = a + d;
}

// one channel of one parent: the children's values v[8] -> the parent's value and the coefficients of the places that hold one
CW_CODEC_HD inline int64_t transform_node_forward(const uint32_t w1[7], const uint32_t w2[7], const int64_t v[8], int64_t d[7]) {
    int64_t z[4], y[2];
    for (int k = 0; k < 4; k++) z[k] = transform_pair(v[2 * k], w1[3 + k], v[2 * k + 1], w2[3 + k], d[3 + k]);
    y[0] = transform_pair(z[0], w1[1], z[1], w2[1], d[1]);
    y[1] = transform_pair(z[2], w1[2], z[3], w2[2], d[2]);
    return transform_pair(y[0], w1[0], y[1], w2[0], d[0]);
}
CW_CODEC_HD inline void transform_node_inverse(const uint32_t w1[7], const uint32_t w2[7], int64_t l, const int64_t d[7], int64_t v[8]) {
    int64_t z[4], y[2];
    transform_unpair(l, w1[0], w2[0], d[0], y[0], y[1]);
    transform_unpair(y[0], w1[1], w2[1], d[1], z[0], z[1]);
    transform_unpair(y[1], w1[2], w2[2], d[2], z[2], z[3]);
    for (int k = 0; k < 4; k++) transform_unpair(z[k], w1[3 + k], w2[3 + k], d[3 + k], v[2 * k], v[2 * k + 1]);
}

// ---------------------------------------------------------------------------
// the container
// ---------------------------------------------------------------------------
struct TransformLayout {
    CodecLayout cwao;                  // the packet this one stands for: 8 colour bits
    uint32_t q16 = TRANSFORM_Q16_MIN;
    int32_t dc[3] = {0, 0, 0};
    uint32_t nescapes[3] = {0, 0, 0};
    int nstreams = 0;
    EntropyStream stream[TRANSFORM_MAX_STREAMS];   // tokens: ENTROPY_BYTES, which = the channel; escapes: TRANSFORM_ESCAPE
    uint64_t directory_offset = 0;     // where the u32 S lies
    uint64_t total_bytes = 0;
};

// The streams that a header and the escape counts imply, in RULE T's order; returns S.
inline int transform_streams(const CodecLayout &l, const uint32_t nescapes[3], EntropyStream s[TRANSFORM_MAX_STREAMS]) {
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
        EntropyStream t;
        t.kind = ENTROPY_BYTES;
        t.which = (uint32_t)ch;
        t.symbols = l.nleaves - 1u;
        t.raw_bytes = t.symbols;
        s[n++] = t;
        EntropyStream e;
        e.kind = TRANSFORM_ESCAPE;
        e.which = (uint32_t)ch;
        e.symbols = nescapes[ch];
        e.raw_bytes = 2u * (uint64_t)nescapes[ch];
        s[n++] = e;
    }
    if (l.tile_mode == 1) {
        EntropyStream e;
        e.kind = ENTROPY_TILE;
        e.symbols = l.nleaves;
        e.raw_bytes = l.nleaves;
        s[n++] = e;
    }
    for (int i = 0; i < n; i++) s[i].nblocks = s[i].kind == TRANSFORM_ESCAPE ? 0u : entropy_block_count(s[i].symbols);
    return n;
}

// The container test: host code, one pass; the coded blocks are not decoded and the tokens are not counted here.
// nullptr: the container is right and `out` filled; otherwise why not.  Nothing outside [p, p + len) is read.
inline const char *transform_validate(const uint8_t *p, size_t len, TransformLayout &out) {
    TransformLayout t;
    CodecLayout &l = t.cwao;
    if (const char *problem = codec_validate_header(p, len, TRANSFORM_MAGIC, l)) return problem;   // (the two versions are both 1)
    if (l.colour_bits != 8) return "colour bits of a transform-coded packet are not 8";
    const uint64_t fixed = CODEC_HEADER_BYTES + 4u * (uint64_t)l.bits;
    if ((uint64_t)len < fixed + TRANSFORM_FIXED_BYTES) return "truncated transform header";
    t.q16 = codec_read<uint16_t>(p + fixed);
    if (t.q16 < TRANSFORM_Q16_MIN || t.q16 > TRANSFORM_Q16_MAX) return "Q16 outside 16..1024";
    for (int ch = 0; ch < 3; ch++) {
        t.dc[ch] = codec_read<int16_t>(p + fixed + 2u + 2u * (uint64_t)ch);
        t.nescapes[ch] = codec_read<uint32_t>(p + fixed + 8u + 4u * (uint64_t)ch);
        if (!l.nleaves && (t.dc[ch] != 0 || t.nescapes[ch] != 0u)) return "dc or escape count of an empty cloud";
        if (l.nleaves && t.nescapes[ch] > l.nleaves - 1u) return "more escapes than coefficients";
    }
    t.directory_offset = fixed + TRANSFORM_FIXED_BYTES;
    t.nstreams = transform_streams(l, t.nescapes, t.stream);
    // an escape stream is always raw (the directory's mode is looked at before RULE E's test reads a table for it)
    if ((uint64_t)len >= t.directory_offset + 4u + 8u * (uint64_t)t.nstreams && codec_read<uint32_t>(p + t.directory_offset) == (uint32_t)t.nstreams)
        for (int i = 0; i < t.nstreams; i++)
            if (t.stream[i].kind == TRANSFORM_ESCAPE && codec_read<uint32_t>(p + t.directory_offset + 4u + 8u * (uint64_t)i) != 0u) return "escape stream is not raw";
    if (const char *problem = entropy_validate_streams(p, len, t.directory_offset, t.nstreams, t.stream, 8, t.total_bytes)) return problem;
    out = t;
    return nullptr;
}

// ---------------------------------------------------------------------------
// the tree and the transform on the host: the kernels' arithmetic, node by node
// ---------------------------------------------------------------------------
// first[i]: the number of inner node i's first child, from the occupancy bytes (inner of them)
inline void transform_first_children(const uint8_t *occupancy, size_t inner, std::vector<uint32_t> &first) {
    first.resize(inner);
    uint32_t at = 1;
    for (size_t i = 0; i < inner; i++) {
        first[i] = at;
        at += (uint32_t)__builtin_popcount(occupancy[i]);
    }
}

// The leaves' 8-bit colours (r, g, b a leaf) -> per channel the zigzag values of the nleaves - 1 quantised coefficients in the
// decoder's order, and dc.
inline void transform_forward(const uint8_t *occupancy, size_t inner, const uint8_t *rgb, uint32_t nleaves, uint32_t q16, std::vector<uint32_t> zz[3], int32_t dc[3]) {
    std::vector<uint32_t> first;
    transform_first_children(occupancy, inner, first);
    const size_t total = inner + nleaves;
    std::vector<uint32_t> weight(total, 1u);
    std::vector<int32_t> value[3];
    for (int ch = 0; ch < 3; ch++) {
        value[ch].assign(total, 0);
        zz[ch].assign(nleaves - 1u, 0u);
    }
    for (uint32_t j = 0; j < nleaves; j++) {
        int32_t v[3];
        transform_to_ycocg(rgb[3 * (size_t)j], rgb[3 * (size_t)j + 1], rgb[3 * (size_t)j + 2], v);
        for (int ch = 0; ch < 3; ch++) value[ch][inner + j] = v[ch];
    }
    for (size_t i = inner; i-- > 0;) {
        uint32_t w[8] = {0}, w1[7], w2[7];
        size_t child = first[i];
        for (int c = 0; c < 8; c++)
            if ((occupancy[i] >> c) & 1) w[c] = weight[child++];
        weight[i] = transform_places(w, w1, w2);
        for (int ch = 0; ch < 3; ch++) {
            int64_t v[8] = {0}, d[7];
            child = first[i];
            for (int c = 0; c < 8; c++)
                if ((occupancy[i] >> c) & 1) v[c] = value[ch][child++];
            value[ch][i] = (int32_t)transform_node_forward(w1, w2, v, d);
            size_t at = (size_t)first[i] - i - 1u;
            const uint32_t q = transform_channel_q16(q16, ch);
            for (int k = 0; k < 7; k++)
                if (w1[k] && w2[k]) zz[ch][at++] = transform_zigzag(transform_quantise(d[k], transform_step(q, w1[k], w2[k])));
        }
    }
    for (int ch = 0; ch < 3; ch++) dc[ch] = value[ch][0];
}

// The inverse: for ANY zz (below 2^17) and dc every value stays far inside int32 (hip_ext.h: Bounds).  rgb: 3 bytes a leaf.
inline void transform_inverse(const uint8_t *occupancy, size_t inner, const std::vector<uint32_t> zz[3], const int32_t dc[3], uint32_t nleaves, uint32_t q16,
                              uint8_t *rgb) {
    std::vector<uint32_t> first;
    transform_first_children(occupancy, inner, first);
    const size_t total = inner + nleaves;
    std::vector<uint32_t> weight(total, 1u);
    for (size_t i = inner; i-- > 0;) {
        uint32_t sum = 0;
        const size_t child = first[i];
        for (int c = 0, k = 0; c < 8; c++)
            if ((occupancy[i] >> c) & 1) sum += weight[child + (size_t)k++];
        weight[i] = sum;
    }
    std::vector<int32_t> value[3];
    for (int ch = 0; ch < 3; ch++) {
        value[ch].assign(total, 0);
        value[ch][0] = dc[ch];
    }
    for (size_t i = 0; i < inner; i++) {
        uint32_t w[8] = {0}, w1[7], w2[7];
        size_t child = first[i];
        for (int c = 0; c < 8; c++)
            if ((occupancy[i] >> c) & 1) w[c] = weight[child++];
        transform_places(w, w1, w2);
        for (int ch = 0; ch < 3; ch++) {
            int64_t v[8], d[7] = {0};
            size_t at = (size_t)first[i] - i - 1u;
            const uint32_t q = transform_channel_q16(q16, ch);
            for (int k = 0; k < 7; k++)
                if (w1[k] && w2[k]) d[k] = transform_unzigzag(zz[ch][at++]) * (int64_t)transform_step(q, w1[k], w2[k]);
            transform_node_inverse(w1, w2, value[ch][i], d, v);
            child = first[i];
            for (int c = 0; c < 8; c++)
                if ((occupancy[i] >> c) & 1) value[ch][child++] = (int32_t)v[c];
        }
    }
    for (uint32_t j = 0; j < nleaves; j++) {
        const uint32_t c = transform_to_rgb(value[0][inner + j], value[1][inner + j], value[2][inner + j]);
        rgb[3 * (size_t)j] = (uint8_t)c;
        rgb[3 * (size_t)j + 1] = (uint8_t)(c >> 8);
        rgb[3 * (size_t)j + 2] = (uint8_t)(c >> 16);
    }
}

// ---------------------------------------------------------------------------
// whole packets on the host
// ---------------------------------------------------------------------------
// a valid "cwao" packet with 8 colour bits, jpeg_quality -> "cwat".  nullptr and `out` filled, or why the input is refused.
inline const char *transform_pack(const uint8_t *p, size_t len, int jpeg_quality, std::vector<uint8_t> &out) {
    CodecLayout l;
    if (const char *problem = codec_validate(p, len, l)) return problem;
    if (l.colour_bits != 8) return "transform coding takes a packet with 8 colour bits";
    if (jpeg_quality < 0 || jpeg_quality > 100) return "jpeg_quality must be in 0..100";
    const uint32_t q16 = transform_q16(jpeg_quality);
    std::vector<uint32_t> zz[3];
    int32_t dc[3] = {0, 0, 0};
    uint32_t nescapes[3] = {0, 0, 0};
    if (l.nleaves) {
        transform_forward(p + l.occupancy_offset, (size_t)l.occupancy_bytes, p + l.colour_offset, l.nleaves, q16, zz, dc);
        for (int ch = 0; ch < 3; ch++)
            for (uint32_t v : zz[ch]) nescapes[ch] += v >= 255u ? 1u : 0u;
    }
    EntropyStream streams[TRANSFORM_MAX_STREAMS];
    const int S = transform_streams(l, nescapes, streams);
    std::vector<std::vector<uint8_t>> payload((size_t)S);
    std::vector<uint8_t> v;
    for (int i = 0; i < S; i++) {
        EntropyStream &s = streams[i];
        if (s.kind == TRANSFORM_ESCAPE) {
            std::vector<uint8_t> &q = payload[(size_t)i];
            q.assign((size_t)codec_pad4(s.raw_bytes), 0);
            size_t at = 0;
            for (uint32_t z : zz[s.which])
                if (z >= 255u) {
                    const uint16_t e = (uint16_t)(z - 255u);
                    memcpy(q.data() + at, &e, 2);
                    at += 2;
                }
            s.mode = 0;
            continue;
        }
        if (!s.symbols) continue;   // (a single leaf has no coefficients: mode 0, an empty payload)
        if (s.kind == ENTROPY_BYTES) {
            v.resize(s.symbols);
            for (uint32_t j = 0; j < s.symbols; j++) v[j] = (uint8_t)(zz[s.which][j] < 255u ? zz[s.which][j] : 255u);
        } else {
            entropy_stream_values(p, l, s, v);
        }
        entropy_make_payload(s, v, 8, payload[(size_t)i]);
    }
    const size_t head = CODEC_HEADER_BYTES + 4u * (size_t)l.bits;
    out.assign(p, p + head);
    const uint32_t magic = TRANSFORM_MAGIC, version = TRANSFORM_VERSION, count = (uint32_t)S;
    memcpy(out.data(), &magic, 4);
    memcpy(out.data() + 4, &version, 4);
    out.resize(head + TRANSFORM_FIXED_BYTES + 4u + 8u * (size_t)S, 0);
    const uint16_t q = (uint16_t)q16;
    memcpy(out.data() + head, &q, 2);
    for (int ch = 0; ch < 3; ch++) {
        const int16_t d = (int16_t)dc[ch];
        memcpy(out.data() + head + 2 + 2 * ch, &d, 2);
        memcpy(out.data() + head + 8 + 4 * ch, &nescapes[ch], 4);
    }
    memcpy(out.data() + head + TRANSFORM_FIXED_BYTES, &count, 4);
    for (int i = 0; i < S; i++) {
        const uint32_t entry[2] = {streams[i].mode, (uint32_t)payload[(size_t)i].size()};
        memcpy(out.data() + head + TRANSFORM_FIXED_BYTES + 4u + 8u * (size_t)i, entry, 8);
    }
    for (int i = 0; i < S; i++) out.insert(out.end(), payload[(size_t)i].begin(), payload[(size_t)i].end());
    return nullptr;
}

// "cwat" -> the "cwao" packet it stands for.  nullptr and `out` filled, or why the packet is refused: the container test, then the
// blocks' integrity, RULE C's two conditions for coded occupancy, and the number of tokens equal to 255 against nescapes.
inline const char *transform_unpack(const uint8_t *p, size_t len, std::vector<uint8_t> &out) {
    TransformLayout t;
    if (const char *problem = transform_validate(p, len, t)) return problem;
    const CodecLayout &l = t.cwao;
    const size_t head = CODEC_HEADER_BYTES + 4u * (size_t)l.bits;
    out.assign((size_t)l.total_bytes, 0);
    memcpy(out.data(), p, head);
    const uint32_t magic = CODEC_MAGIC, version = CODEC_VERSION;
    memcpy(out.data(), &magic, 4);
    memcpy(out.data() + 4, &version, 4);
    if (!l.nleaves) return nullptr;
    std::vector<uint8_t> v;
    std::vector<uint32_t> zz[3];
    for (int i = 0; i < t.nstreams; i++) {
        const EntropyStream &s = t.stream[i];
        if (s.kind == TRANSFORM_ESCAPE) {
            // (the token stream of the channel is the entry before)
            uint32_t taken = 0;
            for (uint32_t &z : zz[s.which])
                if (z == 255u) {
                    if (taken < s.symbols) z += codec_read<uint16_t>(p + s.payload_offset + 2u * (size_t)taken);
                    taken++;
                }
            if (taken != s.symbols) return "tokens equal to 255 differ from the escape count";
            continue;
        }
        if (!s.symbols) continue;
        if (const char *problem = entropy_read_payload(p + s.payload_offset, s, 8, v)) return problem;
        if (s.kind == ENTROPY_OCCUPANCY) {
            memcpy(out.data() + l.occupancy_offset + entropy_depth_offset(l, (int)s.which), v.data(), s.symbols);
        } else if (s.kind == ENTROPY_TILE) {
            memcpy(out.data() + l.tile_offset, v.data(), s.symbols);
        } else {
            zz[s.which].assign(v.begin(), v.end());
        }
    }
    transform_inverse(out.data() + l.occupancy_offset, (size_t)l.occupancy_bytes, zz, t.dc, l.nleaves, t.q16, out.data() + l.colour_offset);
    return nullptr;
}

}  // namespace cwipc_amd
