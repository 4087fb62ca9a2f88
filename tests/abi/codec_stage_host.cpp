// codec_stage_host.cpp -- the octree codec's host staging (csrc/codec_stage.hpp: the stream table under its three plane-offset rules,
// the entropy encoder's work block, RULE T's plane block, the block table of a coded packet, the small terms) as a stand-alone host
// program for tests/test_codec_stage_host.py (built with -fsanitize=address,undefined: every table and block is on the heap and
// exactly as long as the header says, so a step outside it ends the program).
//   codec_stage_host CHECK      one of the checks below; prints what does not hold and returns 1, else prints "ok" and returns 0
#include "codec_stage.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace cwipc_amd;

namespace {

int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            failures++;                                                 \
        }                                                               \
    } while (0)

// a header whose tree is as wide as it can be: nodes[d] = min(8^(d + 1), nleaves)
CodecLayout layout_of(int bits, uint32_t nleaves, int colour_bits, int tile_mode) {
    CodecLayout l;
    l.bits = bits;
    l.nleaves = nleaves;
    l.colour_bits = colour_bits;
    l.tile_mode = tile_mode;
    l.tile_value = tile_mode ? 0 : 5;
    uint64_t wide = 1;
    for (int d = 0; d < bits; d++) {
        wide = std::min<uint64_t>(wide * 8u, nleaves);
        l.nodes[d] = (uint32_t)wide;
    }
    codec_layout_sizes(l);
    return l;
}

struct Case { int bits; uint32_t nleaves; };
// bits 1, 2 and 16; 1 and 2 leaves (RULE T: 0 and 1 coefficients); more than one block of 4096 symbols a stream
const Case CASES[] = {{1, 1}, {1, 2}, {1, 8}, {2, 1}, {2, 2}, {2, 64}, {16, 1}, {16, 2}, {16, 4097}, {16, 30000}};

// what every use of the table has in common
void expect_table(const EntropyStream *s, int n, const k::EntropyStreams &st, size_t capacity) {
    EXPECT(st.nstreams == n);
    uint32_t blocks = 0;
    size_t bytes = 4 + 8u * (size_t)n;
    for (int i = 0; i < n; i++) {
        EXPECT(st.kind[i] == s[i].kind && st.which[i] == s[i].which && st.symbols[i] == s[i].symbols);
        EXPECT(st.first_block[i] == blocks);
        blocks += s[i].nblocks;
        EXPECT(st.raw_padded[i] == (uint32_t)codec_pad4(s[i].raw_bytes));
        bytes += (size_t)codec_pad4(s[i].raw_bytes);
    }
    EXPECT(st.total_blocks == blocks);
    EXPECT(capacity == bytes);
}

// a directory as a packet would carry it, and the decoder's four arrays against it
void expect_decode_arrays(EntropyStream *s, int n, const uint32_t *nodes) {
    const uint64_t directory_offset = 112;
    uint64_t at = directory_offset + 4u + 8u * (uint64_t)n;
    for (int i = 0; i < n; i++) {
        s[i].mode = (uint32_t)(i & 1);
        s[i].payload_offset = at;
        s[i].payload_bytes = codec_pad4(s[i].raw_bytes) + 4u * (uint64_t)i;
        at += s[i].payload_bytes;
    }
    std::unique_ptr<k::EntropyDecode> d(new k::EntropyDecode());
    stage_decode_streams(s, n, directory_offset, *d);
    for (int i = 0; i < n; i++) {
        EXPECT(d->mode[i] == s[i].mode);
        EXPECT(d->payload_offset[i] == (uint32_t)(s[i].payload_offset - directory_offset));
        EXPECT(d->payload_bytes[i] == (uint32_t)s[i].payload_bytes);
        EXPECT(d->children[i] == (s[i].kind == ENTROPY_OCCUPANCY ? nodes[s[i].which] : 0u));   // as the *_streams() lists leave it
    }
}

// RULE E: the encoder (emit_packet) and the decoder (entropy_to_body) list entropy_streams() under stage_offset_rule_e
void streams_rule_e() {
    for (const Case &c : CASES)
        for (int tile_mode = 0; tile_mode < 2; tile_mode++) {
            const CodecLayout l = layout_of(c.bits, c.nleaves, 6, tile_mode);
            EntropyStream s[ENTROPY_MAX_STREAMS];
            const int n = entropy_streams(l, s);
            EXPECT(n == c.bits + 3 + tile_mode && n <= k::ENTROPY_STREAMS);
            std::unique_ptr<k::EntropyStreams> st(new k::EntropyStreams());
            const size_t capacity = stage_streams(s, n, [&](const EntropyStream &es) { return stage_offset_rule_e(l, es); }, *st);
            expect_table(s, n, *st, capacity);
            for (int i = 0; i < n; i++)
                EXPECT(st->plane_offset[i] == (s[i].kind == ENTROPY_OCCUPANCY ? (uint32_t)entropy_depth_offset(l, (int)s[i].which) : 0u));
            expect_decode_arrays(s, n, l.nodes);
        }
    // an empty cloud has no streams: the word S alone
    const CodecLayout empty = layout_of(16, 0, 8, 1);
    EntropyStream s[ENTROPY_MAX_STREAMS];
    std::unique_ptr<k::EntropyStreams> st(new k::EntropyStreams());
    EXPECT(entropy_streams(empty, s) == 0);
    EXPECT(stage_streams(s, 0, [&](const EntropyStream &es) { return stage_offset_rule_e(empty, es); }, *st) == 4 && st->total_blocks == 0);
}

// RULE T: the encoder (emit_packet) and the decoder (decoder_feed_transform) list transform_streams() without its escape streams
// under stage_offset_rule_t
void streams_rule_t() {
    for (const Case &c : CASES)
        for (int tile_mode = 0; tile_mode < 2; tile_mode++) {
            const CodecLayout l = layout_of(c.bits, c.nleaves, 8, tile_mode);
            const size_t ncoef = (size_t)l.nleaves - 1u;
            const uint32_t nescapes[3] = {0, (uint32_t)(ncoef / 2), (uint32_t)ncoef};
            EntropyStream all[TRANSFORM_MAX_STREAMS], s[TRANSFORM_MAX_STREAMS];
            const int nall = transform_streams(l, nescapes, all);
            EXPECT(nall == c.bits + 6 + tile_mode);
            const int n = stage_without_escapes(all, nall, s);
            EXPECT(n == nall - 3 && n <= 20);
            for (int i = 0, j = 0; i < nall; i++)
                if (all[i].kind != TRANSFORM_ESCAPE) {
                    EXPECT(s[j].kind == all[i].kind && s[j].which == all[i].which && s[j].symbols == all[i].symbols && s[j].raw_bytes == all[i].raw_bytes);
                    j++;
                }
            // (the encoder filters in place)
            EXPECT(stage_without_escapes(all, nall, all) == n);
            for (int i = 0; i < n; i++) EXPECT(all[i].kind == s[i].kind && all[i].which == s[i].which);
            std::unique_ptr<k::EntropyStreams> st(new k::EntropyStreams());
            const size_t capacity = stage_streams(s, n, [&](const EntropyStream &es) { return stage_offset_rule_t(l, es); }, *st);
            expect_table(s, n, *st, capacity);
            for (int i = 0; i < n; i++)
                EXPECT(st->plane_offset[i] == (s[i].kind == ENTROPY_OCCUPANCY ? (uint32_t)entropy_depth_offset(l, (int)s[i].which)
                                               : s[i].kind == ENTROPY_BYTES   ? (uint32_t)((size_t)s[i].which * ncoef)
                                                                              : 0u));
            expect_decode_arrays(s, n, l.nodes);
        }
}

// RULE P: the encoder (emit_delta) and the decoder (decoder_feed_delta) list inter_streams() under stage_offset_rule_p
void streams_rule_p() {
    for (const Case &c : CASES)
        for (int tile_mode = 0; tile_mode < 2; tile_mode++)
            for (uint32_t nadded : {0u, 1u, c.nleaves}) {
                const CodecLayout l = layout_of(c.bits, c.nleaves, 5, tile_mode);
                const CodecLayout a = layout_of(c.bits, nadded, 5, tile_mode);   // the tree of the added leaves
                const uint32_t nr = 3 * c.nleaves + 1;
                const size_t n_leaves = l.nleaves, res_offset = stage_round256((nr + 7) / 8);
                EntropyStream s[INTER_MAX_STREAMS];
                const int n = inter_streams(nr, l.nleaves, l.bits, l.colour_bits, tile_mode, nadded, a.nodes, s);
                EXPECT(n == 1 + (nadded ? c.bits : 0) + 3 + tile_mode);
                std::unique_ptr<k::EntropyStreams> st(new k::EntropyStreams());
                const size_t capacity = stage_streams(s, n, [&](const EntropyStream &es) { return stage_offset_rule_p(a.nodes, res_offset, n_leaves, es); }, *st);
                EXPECT(capacity != 0);   // 21 streams at 16 bits with a tile plane: accepted
                expect_table(s, n, *st, capacity);
                for (int i = 0; i < n; i++)
                    EXPECT(st->plane_offset[i] == (s[i].kind == ENTROPY_OCCUPANCY ? (uint32_t)inter_depth_offset(a.nodes, (int)s[i].which)
                                                   : s[i].kind == ENTROPY_BITS    ? (uint32_t)(res_offset + (size_t)s[i].which * n_leaves)
                                                   : s[i].which == 1u             ? (uint32_t)(res_offset + 3 * n_leaves)
                                                                                  : 0u));
                expect_decode_arrays(s, n, a.nodes);
                if (c.bits == 16 && tile_mode == 1 && nadded) EXPECT(n == 21 && n == k::ENTROPY_STREAMS);
            }
}

void stream_count_is_bounded() {
    std::vector<EntropyStream> s(k::ENTROPY_STREAMS + 1);
    for (auto &e : s) {
        e.kind = ENTROPY_BYTES;
        e.symbols = 5000;
        e.nblocks = 2;
        e.raw_bytes = 5000;
    }
    const auto nowhere = [](const EntropyStream &) { return 0u; };
    std::unique_ptr<k::EntropyStreams> st(new k::EntropyStreams());
    st->nstreams = 3;
    st->total_blocks = 7;
    EXPECT(stage_streams(s.data(), k::ENTROPY_STREAMS + 1, nowhere, *st) == 0);   // 22 streams: refused
    EXPECT(st->nstreams == 3 && st->total_blocks == 7);                            // and nothing written
    EXPECT(stage_streams(s.data(), -1, nowhere, *st) == 0);
    const size_t capacity = stage_streams(s.data(), k::ENTROPY_STREAMS, nowhere, *st);   // 21: the tables are full
    EXPECT(capacity == 4 + 8u * 21 + 21u * 5000);
    EXPECT(st->nstreams == 21 && st->total_blocks == 42 && st->first_block[20] == 40);
    // RULE T's list is longer than the tables until its escape streams are out of it
    static_assert(TRANSFORM_MAX_STREAMS > k::ENTROPY_STREAMS && INTER_MAX_STREAMS == k::ENTROPY_STREAMS && ENTROPY_MAX_STREAMS <= k::ENTROPY_STREAMS, "stream bounds");
}

struct Region { const char *name; size_t at, bytes, align; };

// every region inside [0, total), no two overlapping, each aligned
void expect_regions(const std::vector<Region> &regions, size_t total) {
    for (size_t i = 0; i < regions.size(); i++) {
        const Region &r = regions[i];
        if (r.at + r.bytes > total || r.at % r.align) { printf("region %s: [%zu, +%zu) of %zu, alignment %zu\n", r.name, r.at, r.bytes, total, r.align); failures++; }
        for (size_t j = i + 1; j < regions.size(); j++) {
            const Region &o = regions[j];
            if (r.bytes && o.bytes && r.at < o.at + o.bytes && o.at < r.at + r.bytes) { printf("regions %s and %s overlap\n", r.name, o.name); failures++; }
        }
    }
}

void encode_work_layout() {
    const struct { int S; uint32_t blocks; } cases[] = {{1, 1}, {0, 0}, {21, 1}, {21, 5000}};
    for (const auto &c : cases) {
        k::EntropyEncode en{};
        en.st.nstreams = c.S;
        en.st.total_blocks = c.blocks;
        const size_t bytes = stage_encode_work(en, nullptr);
        EXPECT(en.hist == nullptr && en.slots == nullptr);   // the size alone
        // what kernels_entropy.hip's formula asked of the pool before the carve and the size became one function
        const size_t S = (size_t)(c.S ? c.S : 1), nb = c.blocks ? c.blocks : 1;
        EXPECT(bytes <= S * 256 * 4 + S * 256 * 2 + 3 * nb * 4 + S * 12 + 64 + nb * k::ENTROPY_SLOT_BYTES + 1024);
        void *memory = nullptr;
        if (posix_memalign(&memory, 256, bytes ? bytes : 256) != 0) { EXPECT(!"memory"); return; }
        uint8_t *base = (uint8_t *)memory;
        EXPECT(stage_encode_work(en, base) == bytes);
        const size_t s = (size_t)c.S, b = c.blocks;
        const std::vector<Region> regions = {
            {"hist", (size_t)((uint8_t *)en.hist - base), s * 1024, 4},
            {"freq", (size_t)((uint8_t *)en.freq - base), s * 512, 2},
            {"block_words", (size_t)((uint8_t *)en.block_words - base), b * 4, 4},
            {"block_bytes", (size_t)((uint8_t *)en.block_bytes - base), b * 4, 4},
            {"block_offset", (size_t)((uint8_t *)en.block_offset - base), b * 4, 4},
            {"plan", (size_t)((uint8_t *)en.plan - base), s * 12, 4},
            {"report", (size_t)((uint8_t *)en.report - base), 16, 4},
            {"slots", (size_t)(en.slots - base), b * k::ENTROPY_SLOT_BYTES, 256},
        };
        expect_regions(regions, bytes);
        for (const Region &r : regions) memset(base + r.at, 0xa5, r.bytes);   // (the allocation is `bytes` long: the sanitizer watches)
        free(memory);
    }
}

void tree_plane_layout() {
    const struct { size_t inner, nleaves, scan_words; } cases[] = {{1, 1, 16}, {1, 2, 16}, {3, 2, 40}, {431, 1000, 1234}};
    for (const auto &c : cases)
        for (bool encoder : {false, true}) {
            const size_t ncoef = c.nleaves - 1;
            k::TransformTree tree{};
            tree.inner = (uint32_t)c.inner;
            tree.nleaves = (uint32_t)c.nleaves;
            const StageTreePlanes p = stage_tree_planes(tree, nullptr, c.scan_words, encoder);
            EXPECT(tree.first == nullptr && tree.scan == nullptr);   // the sizes alone
            std::vector<uint8_t> block(p.bytes);                     // (exactly the block: the sanitizer watches)
            uint8_t *base = block.data();
            const StageTreePlanes q = stage_tree_planes(tree, base, c.scan_words, encoder);
            EXPECT(q.tokens == p.tokens && q.escapes == p.escapes && q.report == p.report && q.bytes == p.bytes && q.escape_stride == p.escape_stride);
            EXPECT(p.escape_stride >= ncoef && p.escape_stride == ((c.nleaves + 1) & ~(size_t)1));
            std::vector<Region> regions = {
                {"first", (size_t)((uint8_t *)tree.first - base), 4 * c.inner, 256},
                {"weight", (size_t)((uint8_t *)tree.weight - base), 4 * c.inner, 256},
                {"value", (size_t)((uint8_t *)tree.value - base), 12 * (c.inner + c.nleaves), 256},
                {"zz", (size_t)((uint8_t *)tree.zz - base), 12 * ncoef, 256},
                {"scan", (size_t)((uint8_t *)tree.scan - base), 4 * c.scan_words, 256},
                {"tokens", p.tokens, 3 * ncoef, 256},
            };
            if (encoder) {
                regions.push_back({"escapes", p.escapes, 6 * (size_t)p.escape_stride, 256});
                regions.push_back({"report", p.report, 16, 256});
            } else {
                // the planes that encoder and decoder share lie where they lie for both
                k::TransformTree other = tree;
                std::vector<uint8_t> longer(stage_tree_planes(other, nullptr, c.scan_words, true).bytes);
                EXPECT(longer.size() > block.size() && stage_tree_planes(other, longer.data(), c.scan_words, true).tokens == p.tokens);
                EXPECT((uint8_t *)other.first - longer.data() == (uint8_t *)tree.first - base && (uint8_t *)other.weight - longer.data() == (uint8_t *)tree.weight - base &&
                       (uint8_t *)other.value - longer.data() == (uint8_t *)tree.value - base && (uint8_t *)other.zz - longer.data() == (uint8_t *)tree.zz - base &&
                       (uint8_t *)other.scan - longer.data() == (uint8_t *)tree.scan - base);
            }
            expect_regions(regions, p.bytes);
            for (const Region &r : regions) memset(base + r.at, 0xa5, r.bytes);
        }
}

void block_table() {
    // five streams: raw, coded in 2 blocks, raw, coded in 3 blocks, coded in 1 block
    const uint32_t nblocks[5] = {1, 2, 4, 3, 1}, mode[5] = {0, 1, 0, 1, 1};
    const std::vector<std::vector<uint32_t>> sizes = {{}, {260, 8448}, {}, {256, 300, 4096}, {1000}};
    const uint64_t directory_offset = 116;
    EntropyStream s[5];
    uint64_t at = directory_offset + 4u + 8u * 5u;
    std::vector<uint8_t> packet;
    for (int i = 0; i < 5; i++) {
        s[i].kind = ENTROPY_BYTES;
        s[i].nblocks = nblocks[i];
        s[i].symbols = 4096 * nblocks[i];
        s[i].raw_bytes = s[i].symbols;
        s[i].mode = mode[i];
        s[i].payload_offset = at;
        uint64_t bytes = 100;
        if (mode[i]) {
            bytes = ENTROPY_TABLE_BYTES + 4u * nblocks[i];
            for (uint32_t v : sizes[i]) bytes += v;
        }
        s[i].payload_bytes = bytes;
        packet.resize((size_t)(at + bytes), 0xee);
        for (size_t b = 0; b < sizes[i].size(); b++) memcpy(packet.data() + at + ENTROPY_TABLE_BYTES + 4u * b, &sizes[i][b], 4);
        at += bytes;
    }
    std::unique_ptr<k::EntropyStreams> st(new k::EntropyStreams());
    EXPECT(stage_streams(s, 5, [](const EntropyStream &) { return 0u; }, *st) != 0 && st->total_blocks == 11);
    std::vector<uint32_t> table(2 * st->total_blocks, 0xdeadbeefu);   // (exactly the table: the sanitizer watches)
    stage_block_table(s, *st, packet.data(), directory_offset, table.data());
    uint32_t block = 0;
    for (int i = 0; i < 5; i++) {
        uint32_t expect_at = (uint32_t)(s[i].payload_offset - directory_offset) + ENTROPY_TABLE_BYTES + 4u * nblocks[i];   // behind the table and the size words
        for (uint32_t b = 0; b < nblocks[i]; b++, block++) {
            if (!mode[i]) { EXPECT(table[2 * block] == 0 && table[2 * block + 1] == 0); continue; }
            EXPECT(table[2 * block] == expect_at && table[2 * block + 1] == sizes[i][b]);
            expect_at += sizes[i][b];
        }
        if (mode[i]) EXPECT(expect_at == (uint32_t)(s[i].payload_offset + s[i].payload_bytes - directory_offset));   // the blocks fill the payload
    }
    EXPECT(block == st->total_blocks);
}

void decode_terms_follow_the_layout() {
    CodecLayout l = layout_of(16, 30000, 6, 0);
    l.mn[0] = -1.5f; l.mn[1] = 2.25f; l.mn[2] = 1e-3f;
    l.side = 3.5;
    const k::CodecDecode d = stage_decode_terms(l, 16, 6, 0.125);
    EXPECT(d.bits == 16 && d.colour_bits == 6 && d.tile_value == 5 && d.nleaves == 30000 && d.cell == 0.125);
    EXPECT(memcmp(d.nodes, l.nodes, sizeof(d.nodes)) == 0 && memcmp(d.mn, l.mn, sizeof(d.mn)) == 0);
    EXPECT(d.colour_words == codec_pad4(l.colour_bytes) / 4 && d.colours == nullptr && d.tiles == nullptr);
    // the overrides: a cut's bits and cell, RULE T's 8 colour bits
    const k::CodecDecode cut = stage_decode_terms(l, 9, 8, 0.5);
    EXPECT(cut.bits == 9 && cut.colour_bits == 8 && cut.cell == 0.5 && cut.nleaves == 30000 && cut.nodes[15] == l.nodes[15] && cut.tile_value == 5);
    // a delta's header carries neither nodes[] nor offsets
    CodecLayout delta;
    delta.bits = 4;
    delta.colour_bits = 5;
    delta.nleaves = 77;
    const k::CodecDecode p = stage_decode_terms(delta, 4, 5, 1.0);
    EXPECT(p.colour_words == 0 && p.nodes[0] == 0 && p.nodes[3] == 0 && p.nleaves == 77);
}

void tile_words_give_mode_and_value() {
    const uint32_t samples[] = {0u, 1u, 5u, 0x80u, 0xffu, 0x100u, 0xfau, 0x7fu, 0xffffffffu, 0xa5a5a5a5u};
    for (uint32_t w0 : samples)
        for (uint32_t w1 : samples) {
            int mode = -1, value = -1;
            stage_tile_words(w0, w1, mode, value);
            EXPECT(mode == ((w0 & w1) == 0u ? 0 : 1));
            EXPECT(value == ((w0 & w1) == 0u ? (int)(w0 & 255u) : 0));
        }
}

void status_words_give_their_messages() {
    const struct { uint32_t bit; const char *message; } each[] = {
        {1, "entropy-coded block is not intact"},          {2, "occupancy byte is 0"},
        {4, "occupancy bits differ from the node count"},  {16, "padding bits of the kept leaves are not 0"},
        {32, "kept and added leaves differ from the leaf count"}, {8, "an added leaf is a leaf of the reference"},
    };
    EXPECT(stage_refusal(0) == nullptr);
    EXPECT(stage_refusal(64) == nullptr && stage_refusal(0xffffffc0u) == nullptr);   // (no other bit is a status)
    for (size_t i = 0; i < 6; i++) {
        EXPECT(stage_refusal(each[i].bit) != nullptr && strcmp(stage_refusal(each[i].bit), each[i].message) == 0);
        // the order of precedence: 1, 2, 4, 16, 32, 8 -- every earlier bit wins over every later one
        for (size_t j = i + 1; j < 6; j++) EXPECT(strcmp(stage_refusal(each[i].bit | each[j].bit), each[i].message) == 0);
    }
    EXPECT(strcmp(stage_refusal(16u | 8u), "padding bits of the kept leaves are not 0") == 0);
    EXPECT(strcmp(stage_refusal(32u | 8u), "kept and added leaves differ from the leaf count") == 0);
    EXPECT(strcmp(stage_refusal(63u), "entropy-coded block is not intact") == 0);
}

const struct { const char *name; void (*run)(); } CHECKS[] = {
    {"streams_rule_e", streams_rule_e},
    {"streams_rule_t", streams_rule_t},
    {"streams_rule_p", streams_rule_p},
    {"stream_count_is_bounded", stream_count_is_bounded},
    {"encode_work_layout", encode_work_layout},
    {"tree_plane_layout", tree_plane_layout},
    {"block_table", block_table},
    {"decode_terms_follow_the_layout", decode_terms_follow_the_layout},
    {"tile_words_give_mode_and_value", tile_words_give_mode_and_value},
    {"status_words_give_their_messages", status_words_give_their_messages},
};

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2)
        for (const auto &check : CHECKS)
            if (strcmp(argv[1], check.name) == 0) {
                check.run();
                if (failures == 0) printf("ok\n");
                return failures ? 1 : 0;
            }
    fprintf(stderr, "usage: codec_stage_host CHECK, one of:\n");
    for (const auto &check : CHECKS) fprintf(stderr, "  %s\n", check.name);
    return 2;
}
