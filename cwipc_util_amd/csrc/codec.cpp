// codec.cpp -- the octree codec's C boundary and host orchestration: cwipc_hip_new_encoder, cwipc_hip_new_encodergroup,
// cwipc_hip_new_decoder, cwipc_hip_codec_packet_info.  The interface is the one the reference's callers use
// (python/cwipc/net/sink_encoder.py, source_decoder.py); the rule (RULE C: hip_ext.h, codec_terms.hpp) and the packets are this
// library's own and NOT interoperable with cwipc_codec.  The kernels are in kernels_codec.hip.
//
// Encode: filter -> cube, keys, sort, per-depth counts and their scan -> ONE wait (nodes[] and the cube size the packet) -> the
// body's kernels and its copy into page-locked memory, in flight when feed returns.  The header is written by the host; the tile
// mode, known only when the leaves are, is filled in when the result is taken.
// Decode: validate on the host (nothing launched or allocated for a packet that is refused) -> upload -> the kernels, in flight
// when feed returns: the cloud carries a `ready` event.
//
// The entropy-coded form (RULE E: hip_ext.h, entropy_terms.hpp; kernels_entropy.hip).  Encode: the entropy stage runs on the body the
// device holds after codec_leaf; its size is the device's to find, so feed queues the stage and a copy of four report words and
// returns; whoever polls or takes the result first waits for those words and issues the copy of exactly the packet's bytes (EncJob:
// stage 0 -> 1), and takes it when that copy is done.  Decode: the container test on the host -> upload -> the streams decoded into
// the body buffer -> the check -> ONE wait in feed (a packet whose blocks or occupancy bytes fail is refused there) -> the decode above.
//
// Inter-frame coding (RULE P: hip_ext.h, inter_terms.hpp; kernels_inter.hip).  Encode: one wave behind the cube kernel decides between
// key and delta and leaves the cube to quantise in; the choice rides to the host with the cube in the sort's one wait.  A key frame
// is the packet above behind a prefix; its leaves are taken out of the body as the next reference.  A delta frame matches the
// frame's leaves against the reference on the device and WAITS A SECOND TIME for the number of added leaves and their node counts,
// which size the entropy stage's streams; from there on it is the entropy-coded form's path (report, then the copy of exactly the
// packet's bytes).  Decode: the container test on the host -> upload -> the streams decoded, the added keys expanded, the checks ->
// ONE wait -> merge, rebuild, points.  Both keep the frame's leaves on the device with the event of the work that made them.
//
// Transform colour coding (RULE T: hip_ext.h, transform_terms.hpp; kernels_transform.hip).  Encode: behind codec_emit at shift 0 the
// leaves' colours become coefficients, their tokens go through the entropy stage with occupancy and tiles, and one more kernel puts
// the packet together around the escape streams, whose sizes only the device knows; the size arrives as the entropy-coded form's
// does.  Decode: the container test on the host -> upload -> the streams decoded, tokens and escapes joined and counted -> ONE wait ->
// the inverse transform into the body's colour plane -> the decode above.
//
// Level-of-detail decoding (RULE L: hip_ext.h, lod_terms.hpp; kernels_lod.hip).  A decoder told to hand out at most t octree bits does
// everything above up to the packet's body (or, for "cwap", the frame's leaves, which stay the FULL frame as the reference) and then,
// for a packet of b > t bits, makes the cloud of L(P, t) instead of the full one: the leaf runs of the nodes of depth t, the keys of
// depth t alone, the runs' sums, the points.  From a body nothing more is waited for; from a frame's leaves the number of runs is one
// more wait.  cwipc_hip_codec_lod is the host twin: it makes the packet L(P, t).
#include "internal.hpp"
#include "codec_terms.hpp"
#include "entropy_terms.hpp"
#include "inter_terms.hpp"
#include "transform_terms.hpp"
#include "lod_terms.hpp"

#include <cmath>
#include <cstring>
#include <deque>
#include <exception>

using namespace cwipc_amd;

namespace {

size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

struct ErrorbufScope {
    explicit ErrorbufScope(char **errorMessage) { cwipc_log_set_errorbuf(errorMessage); }
    ~ErrorbufScope() { cwipc_log_set_errorbuf(nullptr); }
};

// One encoded packet, possibly still being written by the device.
struct EncJob {
    uint8_t *host = nullptr;
    bool pinned = false;
    CodecLayout layout;              // tile_mode 1 until finalize() has looked at the leaves
    size_t stats_offset = 0;         // where the two tile words land in `host` (0: an empty cloud, nothing in flight)
    hipEvent_t done = nullptr;
    std::shared_ptr<DeviceSoA> src;  // the kernels read its planes
    bool final = false;
    // the entropy-coded form: `out` on the device (from the word S on) until its bytes that count have been copied behind the header
    bool entropy = false, failed = false;
    void *out_dev = nullptr;
    size_t out_capacity = 0, out_bytes = 0, report_offset = 0;
    int stage = 0;                   // 0: the stage's kernels in flight (`done`); 1: the copy in flight (`copied`)
    hipEvent_t copied = nullptr;
    // inter-frame packets: a key packet's prefix lies in front of `host` (the packet starts at host - prefix); a delta packet has
    // the word S at `head` and the header's tile bytes at `tile_at`
    size_t prefix = 0, head = 0, tile_at = 22;
    size_t empty_bytes = 4;          // what an empty cloud has behind its header: S = 0; RULE T: the fixed bytes in front of it
    size_t head_bytes() const { return head ? head : CODEC_HEADER_BYTES + 4u * (size_t)layout.bits; }
    size_t packet_bytes() const { return layout.total_bytes ? prefix + (size_t)layout.total_bytes : 0; }
    ~EncJob() {
        if (done) { (void)hipEventSynchronize(done); event_put(done); }
        if (copied) { (void)hipEventSynchronize(copied); event_put(copied); }
        if (out_dev) pool_free(out_dev);
        if (host) host_free(host - prefix, pinned);
    }
    static bool event_done(hipEvent_t ev, bool wait) {
        if (wait) return hipEventSynchronize(ev) == hipSuccess;
        const hipError_t e = hipEventQuery(ev);
        if (e != hipSuccess) (void)hipGetLastError();
        return e == hipSuccess;
    }
    // `done` has come: the report says how many bytes count; their copy goes out on the calling thread's stream
    void start_copy() {
        stage = 1;
        uint32_t report[4];
        memcpy(report, host + report_offset, 16);
        out_bytes = report[0];
        ThreadCtx &c = tctx();
        if (out_bytes < 4 || out_bytes > out_capacity || !c.ensure()) { failed = true; return; }
        const size_t head = head_bytes();
        copied = event_get();
        if (!copied || hipMemcpyAsync(host + head, out_dev, out_bytes, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
            hipEventRecord(copied, c.stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)c.sync();
            failed = true;
        }
    }
    bool ready(bool wait) {
        if (final || !done) return true;
        if (!entropy) return event_done(done, wait);
        if (stage == 0) {
            if (!event_done(done, wait)) return false;
            start_copy();
        }
        if (failed || !copied) return true;
        return event_done(copied, wait);
    }
    void finalize_entropy() {
        if (done) {
            if (stage == 0) { (void)hipEventSynchronize(done); start_copy(); }
            if (copied) { (void)hipEventSynchronize(copied); event_put(copied); copied = nullptr; }
            event_put(done);
            done = nullptr;
        }
        src.reset();
        if (out_dev) { pool_free(out_dev); out_dev = nullptr; }
        const size_t head = head_bytes();
        layout.tile_mode = 0;
        layout.tile_value = 0;
        if (report_offset) {
            uint32_t report[4];
            memcpy(report, host + report_offset, 16);
            const bool uniform = (report[2] & report[3]) == 0u;
            layout.tile_mode = uniform ? 0 : 1;
            layout.tile_value = uniform ? (int)(report[2] & 255u) : 0;
        } else {
            out_bytes = empty_bytes;   // an empty cloud: S = 0, written with the header
        }
        host[tile_at] = (uint8_t)layout.tile_mode;
        host[tile_at + 1] = (uint8_t)layout.tile_value;
        layout.total_bytes = failed ? 0u : (uint64_t)(head + out_bytes);
        if (failed) note_error("octree encode", "the entropy stage failed");
        final = true;
    }
    void finalize() {
        if (final) return;
        if (entropy) { finalize_entropy(); return; }
        if (done) { (void)hipEventSynchronize(done); event_put(done); done = nullptr; }
        src.reset();
        if (stats_offset) {
            uint32_t stats[2];
            memcpy(stats, host + stats_offset, 8);
            const bool uniform = (stats[0] & stats[1]) == 0u;
            layout.tile_mode = uniform ? 0 : 1;
            layout.tile_value = uniform ? (int)(stats[0] & 255u) : 0;
        } else {
            layout.tile_mode = 0;
            layout.tile_value = 0;
        }
        codec_layout_sizes(layout);
        host[22] = (uint8_t)layout.tile_mode;
        host[23] = (uint8_t)layout.tile_value;
        final = true;
    }
};

// A cloud sorted for `bits`, with what the one read-back brought.
struct Sorted {
    std::shared_ptr<DeviceSoA> src;
    size_t n = 0;
    int bits = 0;
    void *block = nullptr;   // everything below
    unsigned long long *keys = nullptr;
    uint32_t *index = nullptr, *counts = nullptr;
    k::CodecCube *cube_dev = nullptr;
    k::CodecCube cube{{0, 0, 0}, 0, 1.0};
    uint32_t nodes[CODEC_MAX_BITS] = {0};
};

// A frame's leaves on the device as a decoder has them (RULE P's reference), what a delta packet names of it, and the event of the
// work that made it: a feed from another thread's stream waits for that event first.
struct InterRefDev {
    void *block = nullptr;
    k::InterLeavesDev leaves{nullptr, nullptr, nullptr, 0};
    InterReference meta;
    hipEvent_t ready = nullptr;
    ~InterRefDev() {
        if (ready) { (void)hipEventSynchronize(ready); event_put(ready); }
        if (block) pool_free(block);
    }
    static std::unique_ptr<InterRefDev> make(const CodecLayout &l) {
        std::unique_ptr<InterRefDev> r(new InterRefDev());
        const size_t n = l.nleaves, keys_bytes = round256(8 * n);
        uint8_t *block = (uint8_t *)pool_alloc(keys_bytes + 4 * n);
        if (!block) return nullptr;
        r->block = block;
        r->leaves = k::InterLeavesDev{(unsigned long long *)block, block + keys_bytes, block + keys_bytes + 3 * n, l.nleaves};
        r->meta.timestamp = l.timestamp;
        r->meta.nleaves = l.nleaves;
        r->meta.bits = l.bits;
        r->meta.colour_bits = l.colour_bits;
        memcpy(r->meta.mn, l.mn, 12);
        r->meta.side = l.side;
        return r;
    }
    // the work that filled the leaves has been queued on the stream
    bool published(hipStream_t stream) {
        ready = event_get();
        return ready && hipEventRecord(ready, stream) == hipSuccess;
    }
    void wait_on(hipStream_t consumer) const {
        if (ready && hipStreamWaitEvent(consumer, ready, 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipEventSynchronize(ready);
        }
    }
};

// `held` gives way to `next` (may be null); kernels queued on the calling thread's stream may still read the old leaves
void replace_reference(std::unique_ptr<InterRefDev> &held, std::unique_ptr<InterRefDev> next) {
    if (held) {
        tctx().free_later(held->block);
        held->block = nullptr;
    }
    held = std::move(next);
}

// What an inter-mode encoder asks of the sort: the choice between key and delta, made on the device behind the cube kernel.
struct InterAsk {
    bool allow_delta = false;
    float gop_mn[3] = {0, 0, 0};
    double gop_side = 1.0;
    float exp_factor = 1.0f;
    bool delta = false;   // the answer
};

bool sort_cloud(const char *who, const std::shared_ptr<DeviceSoA> &src, int bits, Sorted &out, InterAsk *ask = nullptr) {
    out.src = src;
    out.n = src->npoints;
    out.bits = bits;
    if (out.n == 0) return true;
    if (out.n > 0xfffffff0ull) { note_error(who, "more than 2^32 points"); return false; }
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t n = out.n, nb = k::codec_blocks(n);
    const size_t keys_bytes = round256(2 * n * 8), index_bytes = round256(2 * n * 4), counts_bytes = round256((size_t)bits * (nb + 1) * 4),
                 bounds_bytes = round256(k::codec_bounds_bytes(n));
    uint8_t *block = (uint8_t *)pool_alloc(keys_bytes + index_bytes + counts_bytes + bounds_bytes + 256);
    if (!block) { note_error(who, "out of device memory"); return false; }
    out.block = block;
    out.keys = (unsigned long long *)block;
    out.index = (uint32_t *)(block + keys_bytes);
    out.counts = (uint32_t *)(block + keys_bytes + index_bytes);
    void *partial = block + keys_bytes + index_bytes + counts_bytes;
    out.cube_dev = (k::CodecCube *)(block + keys_bytes + index_bytes + counts_bytes + bounds_bytes);
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, bits);
    k::codec_cube(*src, partial, out.cube_dev, c.stream);
    k::InterCubeReport *inter_report = (k::InterCubeReport *)out.cube_dev;
    if (ask) k::inter_cube(partial, n, inter_report, ask->allow_delta, ask->gop_mn, ask->gop_side, ask->exp_factor, c.stream);
    bool ok = k::codec_sort(*src, out.cube_dev, bits, out.keys, out.index, c.stream);
    if (ok) {
        k::codec_count_scan(out.keys + n, n, out.cube_dev, bits, out.counts, report.device(), tag, c.stream);
        ok = hipMemcpyAsync(c.host_words + 32, out.cube_dev, ask ? sizeof(k::InterCubeReport) : sizeof(k::CodecCube), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = ok && hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;
    ok = ok && report.landed(tag, 0, bits);
    if (!ok) {
        hip_failed(hipGetLastError(), "octree encode (sort)", __FILE__, __LINE__);
        pool_free(block);
        out.block = nullptr;
        return false;
    }
    memcpy(&out.cube, c.host_words + 32, sizeof(k::CodecCube));
    if (ask) {
        k::InterCubeReport got;
        memcpy(&got, c.host_words + 32, sizeof(got));
        ask->delta = got.delta != 0u;
    }
    for (int L = 0; L < bits; L++) out.nodes[L] = report.value(L);
    return true;
}

// the bytes of a packet's body on the device: occupancy, colours, the tile plane, the two tile words
size_t emit_body_bytes(const CodecLayout &l) { return (size_t)(l.tile_offset - l.occupancy_offset) + (size_t)codec_pad4(l.nleaves) + 8; }

// where codec_emit writes in `block` (zeroed): the body, then the leaf sums at sums_offset
k::CodecEmit emit_planes(const CodecLayout &l, uint8_t *block, size_t body_bytes, size_t sums_offset) {
    k::CodecEmit e{};
    e.bits = l.bits;
    e.nleaves = l.nleaves;
    e.depth_offset[0] = 0;
    for (int L = 1; L < l.bits; L++) e.depth_offset[L] = L == 1 ? 1u : e.depth_offset[L - 1] + l.nodes[L - 2];
    e.occupancy_bytes = l.occupancy_bytes;
    e.colour_words = codec_pad4(l.colour_bytes) / 4;
    e.occupancy = (uint32_t *)block;
    e.colours = (uint32_t *)(block + (l.colour_offset - l.occupancy_offset));
    e.tiles = block + (l.tile_offset - l.occupancy_offset);
    e.tile_stats = (uint32_t *)(block + body_bytes - 8);
    e.sums = (k::CodecLeafSum *)(block + sums_offset);
    return e;
}

// the header fields of the packet of (bits, colour shift) from a sorted cloud; tile_mode 1 until the leaves are known
void emit_layout(const Sorted &s, int bits, int shift, uint64_t timestamp, CodecLayout &l) {
    l.timestamp = timestamp;
    l.bits = bits;
    l.colour_bits = 8 - shift;
    l.nleaves = s.n && s.cube.nfinite ? s.nodes[bits - 1] : 0u;
    l.tile_mode = 1;
    if (l.nleaves) {
        for (int L = 0; L < bits; L++) l.nodes[L] = s.nodes[L];
        for (int a = 0; a < 3; a++) l.mn[a] = s.cube.mn[a];
        l.side = s.cube.side;
    }
    codec_layout_sizes(l);
}

// The packet of (bits <= s.bits, colour shift) from a sorted cloud: queued on the calling thread's stream.
// key_leaves (inter mode): the packet is a key packet, `prefix` bytes are kept free in front of it, and the frame's leaves are taken
// out of the body into *key_leaves (sized for the packet's leaf count; unused for an empty cloud).
// transform_q16 != 0 (with entropy, shift 0): the packet is RULE T's, its colours transform coded at that scale.
std::unique_ptr<EncJob> emit_packet(const char *who, const Sorted &s, int bits, int shift, uint64_t timestamp, bool entropy, size_t prefix = 0,
                                    const k::InterLeavesDev *key_leaves = nullptr, uint32_t transform_q16 = 0) {
    ThreadCtx &c = tctx();
    std::unique_ptr<EncJob> job(new EncJob());
    CodecLayout &l = job->layout;
    emit_layout(s, bits, shift, timestamp, l);
    const size_t body_bytes = emit_body_bytes(l);
    // the entropy-coded form: its streams (with a tile plane, which the plan kernel drops when the tiles turn out uniform) and the
    // most bytes it can take from the word S on: a stream never takes more than its raw payload
    k::EntropyStreams st{};
    size_t out_capacity = 4;
    const bool transform = transform_q16 != 0u;
    const size_t ncoef = l.nleaves ? (size_t)l.nleaves - 1u : 0u;
    const uint32_t escape_stride = (uint32_t)(((size_t)l.nleaves + 1u) & ~(size_t)1);   // u16 values a channel: every coefficient, and the padding
    if (entropy) {
        EntropyStream streams[TRANSFORM_MAX_STREAMS];
        if (transform) {
            // RULE T: occupancy, the three token planes and the tile plane go through the stage; the escape streams join them afterwards
            const uint32_t none[3] = {0, 0, 0};
            const int all = transform_streams(l, none, streams);
            for (int i = 0; i < all; i++)
                if (streams[i].kind != TRANSFORM_ESCAPE) streams[st.nstreams++] = streams[i];
        } else {
            st.nstreams = entropy_streams(l, streams);
        }
        st.colour_bits = l.colour_bits;
        st.nleaves = l.nleaves;
        out_capacity += 8u * (size_t)st.nstreams;
        for (int i = 0; i < st.nstreams; i++) {
            st.kind[i] = streams[i].kind;
            st.which[i] = streams[i].which;
            st.symbols[i] = streams[i].symbols;
            st.first_block[i] = st.total_blocks;
            st.total_blocks += streams[i].nblocks;
            st.plane_offset[i] = streams[i].kind == ENTROPY_OCCUPANCY ? (uint32_t)entropy_depth_offset(l, (int)streams[i].which)
                                 : streams[i].kind == ENTROPY_BYTES   ? (uint32_t)((size_t)streams[i].which * ncoef)
                                                                      : 0u;
            st.raw_padded[i] = (uint32_t)codec_pad4(streams[i].raw_bytes);
            out_capacity += st.raw_padded[i];
        }
        if (out_capacity > 0x7fffffffull) { note_error(who, "the cloud is too large for the entropy-coded form"); return nullptr; }
        job->entropy = true;
        job->out_capacity = out_capacity;
        if (transform) {
            // what the packet can take from the fixed bytes on: three more directory entries and every coefficient an escape
            const size_t most = TRANSFORM_FIXED_BYTES + out_capacity + (l.nleaves ? 24u + 3u * (size_t)codec_pad4(2u * ncoef) : 0u);
            if (most > 0x7fffffffull || (uint64_t)l.occupancy_bytes + l.nleaves > 0x7fffffffull) { note_error(who, "the cloud is too large for the transform-coded form"); return nullptr; }
            job->out_capacity = most;
            job->empty_bytes = TRANSFORM_FIXED_BYTES + 4u;
        }
    }
    const size_t entropy_capacity = out_capacity;   // of the entropy stage's own output
    if (entropy) out_capacity = job->out_capacity;
    job->host = (uint8_t *)host_alloc(prefix + (entropy ? (size_t)l.occupancy_offset + out_capacity + 16 : (size_t)l.occupancy_offset + body_bytes), &job->pinned);
    if (!job->host) { note_error(who, "out of host memory"); return nullptr; }
    job->host += prefix;
    job->prefix = prefix;
    codec_write_header(job->host, l);
    if (entropy) {
        const uint32_t magic = transform ? TRANSFORM_MAGIC : ENTROPY_MAGIC, none = 0;
        memcpy(job->host, &magic, 4);
        memcpy(job->host + l.occupancy_offset, &none, 4);
        if (transform) {   // (an empty cloud's packet ends with these bytes)
            const uint16_t q = (uint16_t)transform_q16;
            memset(job->host + l.occupancy_offset, 0, TRANSFORM_FIXED_BYTES + 4u);
            memcpy(job->host + l.occupancy_offset, &q, 2);
        }
    }
    if (!l.nleaves) {
        job->finalize();
        return job;
    }
    if (!c.ensure()) return nullptr;
    const size_t sums_offset = (body_bytes + 7) & ~(size_t)7, block_bytes = sums_offset + (size_t)l.nleaves * sizeof(k::CodecLeafSum);
    uint8_t *block = (uint8_t *)pool_alloc(block_bytes);
    if (!block) { note_error(who, "out of device memory"); return nullptr; }
    const k::CodecEmit e = emit_planes(l, block, body_bytes, sums_offset);
    uint8_t *work = nullptr, *tblock = nullptr, *stage_out = nullptr;
    // RULE T's planes: first, weight, the values, the zigzag values, the scans' words, the tokens, the escapes, the report
    k::TransformTree tree{};
    size_t tokens_at = 0, escapes_at = 0, treport_at = 0;
    if (transform) {
        k::transform_tree_counts(tree, l.bits, l.nodes, l.nleaves, transform_q16);
        const size_t inner = tree.inner, total = inner + l.nleaves;
        const size_t first_at = 0, weight_at = first_at + round256(4 * inner), value_at = weight_at + round256(4 * inner), zz_at = value_at + round256(12 * total),
                     scan_at = zz_at + round256(12 * ncoef + 4);
        tokens_at = scan_at + round256(4 * k::transform_scan_words(tree));
        escapes_at = tokens_at + round256(3 * ncoef + 4);
        treport_at = escapes_at + round256(6 * (size_t)escape_stride);
        tblock = (uint8_t *)pool_alloc(treport_at + 256);
        if (tblock) {
            tree.first = (uint32_t *)(tblock + first_at);
            tree.weight = (uint32_t *)(tblock + weight_at);
            tree.value = (int32_t *)(tblock + value_at);
            tree.zz = (uint32_t *)(tblock + zz_at);
            tree.scan = (uint32_t *)(tblock + scan_at);
        }
    }
    if (entropy) {
        work = (uint8_t *)pool_alloc(k::entropy_encode_work_bytes(st));
        job->out_dev = pool_alloc(round256(out_capacity));
        if (transform) stage_out = (uint8_t *)pool_alloc(round256(entropy_capacity));
        if (!work || !job->out_dev || (transform && (!tblock || !stage_out))) {
            pool_free(work);
            pool_free(block);
            pool_free(tblock);
            pool_free(stage_out);
            note_error(who, "out of device memory");
            return nullptr;
        }
    }
    bool ok = hipMemsetAsync(block, 0, block_bytes, c.stream) == hipSuccess;
    if (ok) {
        k::codec_emit(s.keys + s.n, s.index + s.n, *s.src, s.cube_dev, s.bits, s.counts, e, shift, c.stream);
        if (key_leaves) k::inter_leaves_of_body(s.keys + s.n, s.n, s.cube_dev, s.counts, e, l.colour_bits, *key_leaves, c.stream);
        if (!entropy) ok = hipMemcpyAsync(job->host + l.occupancy_offset, block, body_bytes, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = ok && hipGetLastError() == hipSuccess;
    }
    if (ok && entropy) {
        // only the packet's own bytes cross the bus: here the four report words, the rest when the result is polled or taken
        k::EntropyEncode en{};
        en.st = st;
        en.occupancy = (const uint8_t *)e.occupancy;
        en.tiles = e.tiles;
        en.colours = e.colours;
        en.tile_stats = e.tile_stats;
        en.colour_words = e.colour_words;
        const size_t S = (size_t)st.nstreams, nb = st.total_blocks;
        uint8_t *at = work;
        en.hist = (uint32_t *)at; at += S * 1024;
        en.block_words = (uint32_t *)at; at += nb * 4;
        en.block_bytes = (uint32_t *)at; at += nb * 4;
        en.block_offset = (uint32_t *)at; at += nb * 4;
        en.plan = (uint32_t *)at; at += S * 12;
        en.report = (uint32_t *)at; at += 16;
        en.freq = (uint16_t *)at; at += S * 512;
        en.slots = work + round256((size_t)(at - work));
        en.out = transform ? stage_out : (uint8_t *)job->out_dev;
        en.out_capacity = entropy_capacity;
        job->report_offset = (size_t)l.occupancy_offset + (size_t)codec_pad4(out_capacity);
        ok = hipMemsetAsync(en.hist, 0, S * 1024, c.stream) == hipSuccess && hipMemsetAsync(en.out, 0, entropy_capacity, c.stream) == hipSuccess;
        const uint32_t *report = en.report;
        if (ok && transform) {
            // the coefficients of the leaves' colours, their tokens as the stage's byte planes, and the packet put together behind it
            tree.occupancy = en.occupancy;
            uint8_t *tokens = tblock + tokens_at;
            uint16_t *escapes = (uint16_t *)(tblock + escapes_at);
            ok = hipMemsetAsync(escapes, 0, 6 * (size_t)escape_stride, c.stream) == hipSuccess;
            k::transform_prepare(tree, c.stream);
            k::transform_forward(tree, (const uint8_t *)e.colours, c.stream);
            k::transform_tokens(tree, tokens, escapes, escape_stride, c.stream);
            en.planes = tokens;
            k::entropy_encode(en, c.stream);
            k::TransformAssemble a{};
            a.bits = l.bits;
            a.entropy_streams = st.nstreams;
            a.plan = en.plan;
            a.in_report = en.report;
            a.in = en.out;
            a.escapes = escapes;
            a.escape_stride = escape_stride;
            for (int ch = 0; ch < 3; ch++) {
                a.escape_total[ch] = k::transform_escape_total(tree, ch);
                a.dc[ch] = tree.value + (size_t)ch * ((size_t)tree.inner + l.nleaves);
            }
            a.q16 = transform_q16;
            a.out = (uint8_t *)job->out_dev;
            a.out_capacity = out_capacity;
            a.report = (uint32_t *)(tblock + treport_at);
            k::transform_assemble(a, c.stream);
            report = a.report;
        } else if (ok) {
            k::entropy_encode(en, c.stream);
        }
        if (ok) {
            ok = hipMemcpyAsync(job->host + job->report_offset, report, 16, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
            ok = ok && hipGetLastError() == hipSuccess;
        }
    }
    job->done = event_get();
    ok = ok && job->done && hipEventRecord(job->done, c.stream) == hipSuccess;
    c.free_later(block);
    c.free_later(work);
    c.free_later(tblock);
    c.free_later(stage_out);
    if (!ok) {
        (void)c.sync();
        hip_failed(hipGetLastError(), "octree encode", __FILE__, __LINE__);
        return nullptr;
    }
    if (!entropy) job->stats_offset = (size_t)l.occupancy_offset + body_bytes - 8;
    job->src = s.src;
    return job;
}

// The delta packet (RULE P) of the sorted cloud's frame against the reference R, queued on the calling thread's stream after a wait
// of its own for the number of added leaves and their node counts.  The frame's leaves go to P (sized for its leaf count, above 0).
std::unique_ptr<EncJob> emit_delta(const char *who, const Sorted &s, int bits, int shift, uint64_t timestamp, uint32_t gop_index, const InterRefDev &R,
                                   const k::InterLeavesDev &P) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    std::unique_ptr<EncJob> job(new EncJob());
    CodecLayout &l = job->layout;
    emit_layout(s, bits, shift, timestamp, l);
    const size_t n = l.nleaves, nr = R.leaves.n, nb = k::codec_blocks(n);
    const size_t body_bytes = emit_body_bytes(l), sums_offset = (body_bytes + 7) & ~(size_t)7, body_block_bytes = sums_offset + n * sizeof(k::CodecLeafSum);
    // the planes the entropy stage reads: keep, then the four residual planes; behind them what the match and the count of A need
    const size_t keep_bytes = (nr + 7) / 8, res_offset = round256(keep_bytes), added_offset = res_offset + round256(4 * n),
                 counts_offset = added_offset + round256(9 * n), counts_added_offset = counts_offset + round256((nb + 1) * 4),
                 cube_offset = counts_added_offset + round256((size_t)bits * (nb + 1) * 4), match_bytes = cube_offset + 256;
    if (match_bytes > 0x7fffffffull) { note_error(who, "the cloud is too large for a delta packet"); return nullptr; }
    // (given back by hand: a block handed to free_later would return to the pool in the wait below)
    struct Blocks {
        uint8_t *body = nullptr, *match = nullptr, *occupancy = nullptr, *work = nullptr;
        bool queued = false;   // kernels that read them are in flight on the calling thread's stream
        ~Blocks() {
            for (uint8_t *p : {body, match, occupancy, work})
                if (queued) tctx().free_later(p); else pool_free(p);
        }
    } blocks;
    blocks.body = (uint8_t *)pool_alloc(body_block_bytes);
    blocks.match = (uint8_t *)pool_alloc(match_bytes);
    if (!blocks.body || !blocks.match) { note_error(who, "out of device memory"); return nullptr; }
    uint8_t *match = blocks.match;
    const k::CodecEmit e = emit_planes(l, blocks.body, body_bytes, sums_offset);
    unsigned long long *added = (unsigned long long *)(match + added_offset);
    uint32_t *counts_added = (uint32_t *)(match + counts_added_offset);
    k::CodecCube *cube_added = (k::CodecCube *)(match + cube_offset);
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 17);   // words 0 .. bits - 1: nodesA[]; word 16: nadded
    bool ok = hipMemsetAsync(blocks.body, 0, body_block_bytes, c.stream) == hipSuccess;
    if (ok) {
        k::codec_emit(s.keys + s.n, s.index + s.n, *s.src, s.cube_dev, s.bits, s.counts, e, shift, c.stream);
        k::inter_leaves_of_body(s.keys + s.n, s.n, s.cube_dev, s.counts, e, l.colour_bits, P, c.stream);
        k::inter_match(R.leaves, P, l.colour_bits, match, match + res_offset, added, (uint32_t *)(match + counts_offset), cube_added, report.device() + 16, tag,
                       c.stream);
        k::codec_count_scan(added, n, cube_added, bits, counts_added, report.device(), tag, c.stream);
        ok = hipMemcpyAsync(c.host_words + 40, e.tile_stats, 8, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = ok && hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;   // the second wait of a delta frame
    ok = ok && report.landed(tag, 0, bits) && report.landed(tag, 16);
    if (!ok) {
        hip_failed(hipGetLastError(), "octree encode (match)", __FILE__, __LINE__);
        return nullptr;
    }
    const uint32_t nadded = report.value(16);
    uint32_t nodes_added[CODEC_MAX_BITS] = {0};
    for (int L = 0; L < bits; L++) nodes_added[L] = report.value(L);
    uint32_t stats[2];
    memcpy(stats, c.host_words + 40, 8);
    const bool uniform = (stats[0] & stats[1]) == 0u;
    l.tile_mode = uniform ? 0 : 1;
    l.tile_value = uniform ? (int)(stats[0] & 255u) : 0;
    if (nadded > n || (nadded ? nodes_added[bits - 1] != nadded : nodes_added[bits - 1] != 0u)) { note_error(who, "the match lost count of the added leaves"); return nullptr; }
    // the streams, now that every count is known, and the most bytes the packet can take from the word S on
    EntropyStream streams[INTER_MAX_STREAMS];
    k::EntropyStreams st{};
    st.nstreams = inter_streams((uint32_t)nr, l.nleaves, bits, l.colour_bits, l.tile_mode, nadded, nodes_added, streams);
    st.colour_bits = l.colour_bits;
    st.nleaves = l.nleaves;
    size_t out_capacity = 4 + 8u * (size_t)st.nstreams;
    for (int i = 0; i < st.nstreams; i++) {
        const EntropyStream &es = streams[i];
        st.kind[i] = es.kind;
        st.which[i] = es.which;
        st.symbols[i] = es.symbols;
        st.first_block[i] = st.total_blocks;
        st.total_blocks += es.nblocks;
        st.plane_offset[i] = es.kind == ENTROPY_OCCUPANCY ? (uint32_t)inter_depth_offset(nodes_added, (int)es.which)
                             : es.kind == ENTROPY_BITS    ? (uint32_t)(res_offset + (size_t)es.which * n)
                             : es.which == 1u             ? (uint32_t)(res_offset + 3 * n)
                                                          : 0u;
        st.raw_padded[i] = (uint32_t)codec_pad4(es.raw_bytes);
        out_capacity += st.raw_padded[i];
    }
    if (out_capacity > 0x7fffffffull) { note_error(who, "the cloud is too large for a delta packet"); return nullptr; }
    const size_t head = INTER_PREFIX_BYTES + INTER_HEADER_BYTES + 4u + 4u * (size_t)bits;
    job->entropy = true;
    job->out_capacity = out_capacity;
    job->head = head;
    job->tile_at = INTER_PREFIX_BYTES + 22 - 8;
    job->report_offset = head + (size_t)codec_pad4(out_capacity);
    job->host = (uint8_t *)host_alloc(job->report_offset + 16, &job->pinned);
    if (!job->host) { note_error(who, "out of host memory"); return nullptr; }
    uint8_t header[CODEC_HEADER_BYTES + 4 * CODEC_MAX_BITS];
    codec_write_header(header, l);
    inter_write_prefix(job->host, INTER_DELTA, gop_index, R.meta.timestamp, R.meta.nleaves);
    memcpy(job->host + INTER_PREFIX_BYTES, header + 8, INTER_HEADER_BYTES);
    memcpy(job->host + INTER_PREFIX_BYTES + INTER_HEADER_BYTES, &nadded, 4);
    memcpy(job->host + INTER_PREFIX_BYTES + INTER_HEADER_BYTES + 4, nodes_added, 4u * (size_t)bits);
    // the occupancy bytes of the added leaves
    uint64_t depth_offset[CODEC_MAX_BITS] = {0};
    for (int L = 0; L < bits; L++) depth_offset[L] = inter_depth_offset(nodes_added, L);
    const uint64_t occupancy_bytes = nadded ? depth_offset[bits - 1] + (bits > 1 ? nodes_added[bits - 2] : 1u) : 0u;
    const size_t occupancy_block = round256((size_t)codec_pad4(occupancy_bytes) + 4);
    blocks.occupancy = (uint8_t *)pool_alloc(occupancy_block);
    blocks.work = (uint8_t *)pool_alloc(k::entropy_encode_work_bytes(st));
    job->out_dev = pool_alloc(round256(out_capacity));
    if (!blocks.occupancy || !blocks.work || !job->out_dev) { note_error(who, "out of device memory"); return nullptr; }
    k::EntropyEncode en{};
    en.st = st;
    en.planes = match;
    en.occupancy = blocks.occupancy;
    en.tile_stats = e.tile_stats;
    const size_t S = (size_t)st.nstreams, nblocks = st.total_blocks;
    uint8_t *at = blocks.work;
    en.hist = (uint32_t *)at; at += S * 1024;
    en.block_words = (uint32_t *)at; at += nblocks * 4;
    en.block_bytes = (uint32_t *)at; at += nblocks * 4;
    en.block_offset = (uint32_t *)at; at += nblocks * 4;
    en.plan = (uint32_t *)at; at += S * 12;
    en.report = (uint32_t *)at; at += 16;
    en.freq = (uint16_t *)at; at += S * 512;
    en.slots = blocks.work + round256((size_t)(at - blocks.work));
    en.out = (uint8_t *)job->out_dev;
    en.out_capacity = out_capacity;
    blocks.queued = true;
    ok = hipMemsetAsync(blocks.occupancy, 0, occupancy_block, c.stream) == hipSuccess && hipMemsetAsync(en.hist, 0, S * 1024, c.stream) == hipSuccess &&
         hipMemsetAsync(job->out_dev, 0, out_capacity, c.stream) == hipSuccess;
    if (ok) {
        k::inter_occupancy(added, nadded, n, bits, counts_added, depth_offset, occupancy_bytes, (uint32_t *)blocks.occupancy, c.stream);
        k::entropy_encode(en, c.stream);
        ok = hipMemcpyAsync(job->host + job->report_offset, en.report, 16, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = ok && hipGetLastError() == hipSuccess;
    }
    job->done = event_get();
    ok = ok && job->done && hipEventRecord(job->done, c.stream) == hipSuccess;
    if (!ok) {
        (void)c.sync();
        hip_failed(hipGetLastError(), "octree encode (delta)", __FILE__, __LINE__);
        return nullptr;
    }
    job->src = s.src;
    return job;
}

// The cloud an encoder of (tilenumber, voxelsize) works on, on the device.  `made` receives the clouds made on the way.
std::shared_ptr<DeviceSoA> filtered_input(const char *who, cwipc_pointcloud *pc, int tilenumber, float voxelsize, std::vector<cwipc_pointcloud *> &made,
                                          std::unique_ptr<cwipc_hip_pointcloud> &keep) {
    cwipc_pointcloud *cur = pc;
    if (tilenumber != 0) {
        cur = cwipc_tilefilter(cur, tilenumber);
        if (!cur) { note_error(who, "cwipc_tilefilter failed"); return nullptr; }
        made.push_back(cur);
    }
    if (voxelsize > 0) {
        cur = cwipc_downsample(cur, voxelsize);
        if (!cur) { note_error(who, "cwipc_downsample failed"); return nullptr; }
        made.push_back(cur);
    }
    cwipc_hip_pointcloud *ours = as_ours(cur);
    if (!ours) {
        keep = import_foreign(cur);
        ours = keep.get();
    }
    if (!ours || !ours->has_data()) { note_error(who, "cannot read the point data of the argument"); return nullptr; }
    if (!device_available(who)) return nullptr;
    auto dev = ours->device_points();
    if (!dev) note_error(who, "the cloud cannot be brought to the device");
    return dev;
}

// The clouds filtered_input made on the way: they go when the feed that asked for them is over (the planes stay with the packet's job).
struct MadeClouds {
    std::vector<cwipc_pointcloud *> list;
    ~MadeClouds() { for (cwipc_pointcloud *p : list) delete p; }
};

// No exception crosses the C boundary: what the standard library throws in a call's body (memory) is logged and becomes its error value.
template <typename T, typename Body>
T guarded(const char *who, T failed, Body &&body) {
    try {
        return body();
    } catch (const std::exception &e) {
        note_error(who, e.what());
    } catch (...) {
        note_error(who, "unknown exception");
    }
    return failed;
}

const char *params_problem(const cwipc_hip_encoder_params &p) {
    if (!inter_params_on(p.do_inter_frame, p.gop_size, p.exp_factor)) {
        if (p.do_inter_frame) return "do_inter_frame needs gop_size in 2..65535 and exp_factor in 1..16 with it (RULE P)";
        if (p.gop_size != 1) return "gop_size must be 1 (inter mode: do_inter_frame with gop_size in 2..65535 and exp_factor in 1..16)";
        if (!(p.exp_factor == 1.0f)) return "exp_factor must be 1.0 (inter mode: do_inter_frame with gop_size in 2..65535 and exp_factor in 1..16)";
    }
    if (p.octree_bits < 1 || p.octree_bits > CODEC_MAX_BITS) return "octree_bits must be in 1..16";
    if (p.jpeg_quality < 0 || p.jpeg_quality > 100) return "jpeg_quality must be in 0..100";
    if (std::isnan(p.voxelsize)) return "voxelsize is not a number";
    return nullptr;
}

}  // namespace

struct cwipc_hip_encoder {
    cwipc_hip_encoder_params params;
    std::mutex lock;
    std::deque<std::unique_ptr<EncJob>> queue;
    bool closed = false;
    bool in_group = false;
    bool entropy = false;   // deliver the entropy-coded form (RULE E); chosen before the first feed
    bool transform = false; // deliver RULE T's form ("cwat"): the colours transform coded, the rest as under RULE E
    bool fed = false;
    // inter mode (RULE P): the sequence, the GOP's cube and the reference, under a lock of their own that a feed holds throughout
    bool inter = false;
    std::mutex inter_lock;
    InterSequence sequence;
    float gop_mn[3] = {0, 0, 0};
    double gop_side = 1.0;
    std::unique_ptr<InterRefDev> reference;
};

struct cwipc_hip_encodergroup {
    std::mutex lock;
    std::vector<cwipc_hip_encoder *> encoders;
};

struct cwipc_hip_decoder {
    struct Job {
        cwipc_pointcloud *cloud = nullptr;
        std::shared_ptr<DeviceSoA> planes;   // (its `ready` event says when the kernels are done)
        uint8_t *host = nullptr;             // the packet as the upload reads it
        bool pinned = false;
    };
    std::mutex lock;
    std::deque<Job> queue;
    bool closed = false;
    // the frame of the last "cwap" packet (RULE P), under a lock of its own that a feed of such a packet holds throughout
    std::mutex inter_lock;
    std::unique_ptr<InterRefDev> reference;
    std::atomic<int> max_bits{0};   // RULE L: 0, or the most octree bits of a cloud handed out; read once a feed
};

namespace {

// the octree bits of the cloud a decoder with `max_bits` hands out for a packet of `bits`
int lod_out_bits(int bits, int max_bits) { return max_bits > 0 && bits > max_bits ? max_bits : bits; }

// RULE L from a packet's body on the device (occupancy bytes at `body`; `full`: the decode of all l.bits, its colour and tile planes
// in place): the cloud of L(P, t), t < l.bits, into dst (l.nodes[t - 1] points), queued on the calling thread's stream.
// first: the tree's first children where the caller has them (transform_prepare), or nullptr: made here.
bool lod_from_body(const char *who, ThreadCtx &c, const uint8_t *body, const CodecLayout &l, const k::CodecDecode &full, int t, const uint32_t *first,
                   const DeviceSoA &dst) {
    const uint32_t nruns = l.nodes[t - 1];
    if ((uint64_t)l.occupancy_bytes + l.nleaves > 0x7fffffffull) { note_error(who, "the packet is too large for level-of-detail decoding"); return false; }   // (the tree's node numbers are 32 bits)
    k::TransformTree tree{};
    k::transform_tree_counts(tree, l.bits, l.nodes, l.nleaves, TRANSFORM_Q16_MIN);
    k::CodecDecode d = full;
    d.bits = t;
    d.nleaves = nruns;
    d.cell = codec_cellsize(l.side, t);
    const size_t first_bytes = first ? 0 : round256(4 * (size_t)tree.inner), scan_bytes = first ? 0 : round256(4 * k::transform_scan_words(tree)),
                 start_bytes = round256(4 * ((size_t)nruns + 1)), ping_bytes = round256(8 * (size_t)nruns), scratch_bytes = round256(k::codec_decode_scratch_words(d) * 4),
                 sums_bytes = round256((size_t)nruns * sizeof(k::CodecLeafSum));
    uint8_t *block = (uint8_t *)pool_alloc(first_bytes + scan_bytes + start_bytes + 2 * ping_bytes + scratch_bytes + sums_bytes);
    if (!block) { note_error(who, "out of device memory"); return false; }
    uint8_t *at = block;
    if (!first) {
        tree.occupancy = body;
        tree.first = (uint32_t *)at; at += first_bytes;
        tree.scan = (uint32_t *)at; at += scan_bytes;
        k::transform_prepare(tree, c.stream);
        first = tree.first;
    }
    uint32_t *start = (uint32_t *)at; at += start_bytes;
    unsigned long long *ping = (unsigned long long *)at, *pong = (unsigned long long *)(at + ping_bytes); at += 2 * ping_bytes;
    uint32_t *scratch = (uint32_t *)at; at += scratch_bytes;
    k::lod_runs_of_tree(first, tree.inner, tree.depth_begin[t], l.bits - t, nruns, l.nleaves, start, c.stream);
    const unsigned long long *cut = k::codec_expand(body, d, ping, pong, scratch, c.stream);
    const k::LodSource src{l.nleaves, full.colour_bits, full.tile_value, full.colours, full.colour_words, nullptr, full.tiles};
    const bool ok = k::lod_points(src, start, nruns, cut, (k::CodecLeafSum *)at, d, dst, c.stream);
    c.free_later(block);
    return ok;
}

// RULE L from a frame's leaves on the device (RULE P's reference, the full frame of l.bits): the cloud of L(P, t), t < l.bits, after
// ONE wait for the number of its points.  nullptr: failed (logged).
std::shared_ptr<DeviceSoA> lod_from_leaves(const char *who, ThreadCtx &c, const k::InterLeavesDev &leaves, const CodecLayout &l, int t) {
    const size_t n = leaves.n;
    const size_t start_bytes = round256(4 * (n + 1)), cut_bytes = round256(8 * n), counts_bytes = round256(4 * k::lod_key_runs_words(n));
    uint8_t *block = (uint8_t *)pool_alloc(start_bytes + cut_bytes + counts_bytes);
    if (!block) { note_error(who, "out of device memory"); return nullptr; }
    uint32_t *start = (uint32_t *)block;
    unsigned long long *cut = (unsigned long long *)(block + start_bytes);
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 1);
    k::lod_runs_of_keys(leaves.keys, leaves.n, l.bits, t, start, cut, (uint32_t *)(block + start_bytes + cut_bytes), report.device(), tag, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = c.sync() && ok;   // the wait: how many points the cloud has
    ok = ok && report.landed(tag, 0);
    const uint32_t nruns = ok ? report.value(0) : 0u;
    if (!ok || nruns < 1 || nruns > n) {
        pool_free(block);
        if (!ok) hip_failed(hipGetLastError(), "octree decode (level of detail)", __FILE__, __LINE__);
        else note_error(who, "the leaf runs lost count");
        return nullptr;
    }
    auto dst = soa_alloc(nruns);
    k::CodecLeafSum *sums = (k::CodecLeafSum *)pool_alloc(round256((size_t)nruns * sizeof(k::CodecLeafSum)));
    if (!dst || !sums) {
        pool_free(block);
        pool_free(sums);
        note_error(who, "out of device memory");
        return nullptr;
    }
    k::CodecDecode d{};
    d.bits = t;
    d.colour_bits = l.colour_bits;
    d.nleaves = nruns;
    for (int a = 0; a < 3; a++) d.mn[a] = l.mn[a];
    d.cell = codec_cellsize(l.side, t);
    const k::LodSource src{leaves.n, l.colour_bits, 0, nullptr, 0, leaves.colour, leaves.tiles};
    ok = k::lod_points(src, start, nruns, cut, sums, d, *dst, c.stream) && hipGetLastError() == hipSuccess;
    c.free_later(block);
    c.free_later(sums);
    if (!ok) {
        (void)c.sync();
        hip_failed(hipGetLastError(), "octree decode (level of detail)", __FILE__, __LINE__);
        return nullptr;
    }
    return dst;
}

void release_upload(cwipc_hip_decoder::Job &j) {
    if (j.host) {
        if (j.planes) j.planes->wait_host();
        host_free(j.host, j.pinned);
        j.host = nullptr;
    }
}

// The streams of a "cwae" packet that has passed entropy_validate() into `body`, the device copy of the "cwao" body that the octree
// decoder reads: upload, decode, check, and the one wait for the check's word.  False (logged): a block is not intact or a coded
// occupancy stream breaks RULE C; the caller launches nothing more for the packet.
bool entropy_to_body(const char *who, ThreadCtx &c, const uint8_t *bytes, const EntropyLayout &el, uint8_t *body) {
    const CodecLayout &l = el.cwao;
    k::EntropyDecode d{};
    d.st.nstreams = el.nstreams;
    d.st.colour_bits = l.colour_bits;
    d.st.nleaves = l.nleaves;
    for (int i = 0; i < el.nstreams; i++) {
        const EntropyStream &s = el.stream[i];
        d.st.kind[i] = s.kind;
        d.st.which[i] = s.which;
        d.st.symbols[i] = s.symbols;
        d.st.first_block[i] = d.st.total_blocks;
        d.st.total_blocks += s.nblocks;
        d.st.plane_offset[i] = s.kind == ENTROPY_OCCUPANCY ? (uint32_t)entropy_depth_offset(l, (int)s.which) : 0u;
        d.st.raw_padded[i] = (uint32_t)codec_pad4(s.raw_bytes);
        d.mode[i] = s.mode;
        d.payload_offset[i] = (uint32_t)(s.payload_offset - el.directory_offset);
        d.payload_bytes[i] = (uint32_t)s.payload_bytes;
        d.children[i] = s.kind == ENTROPY_OCCUPANCY ? l.nodes[s.which] : 0u;
    }
    const size_t in_bytes = (size_t)(el.total_bytes - el.directory_offset), table_offset = (in_bytes + 7) & ~(size_t)7,
                 table_bytes = 8u * (size_t)d.st.total_blocks, upload_bytes = round256(table_offset + table_bytes),
                 channel_bytes = round256(3u * (size_t)l.nleaves), flag_bytes = round256(4u * (size_t)(1 + el.nstreams));
    bool pinned = false;
    uint8_t *host = (uint8_t *)host_alloc(upload_bytes, &pinned);
    uint8_t *dev = (uint8_t *)pool_alloc(upload_bytes + channel_bytes + flag_bytes);
    if (!host || !dev) {
        if (host) host_free(host, pinned);
        pool_free(dev);
        note_error(who, "out of memory");
        return false;
    }
    memcpy(host, bytes + el.directory_offset, in_bytes);
    uint32_t *table = (uint32_t *)(host + table_offset);
    memset(table, 0, table_bytes);
    for (int i = 0; i < el.nstreams; i++) {
        const EntropyStream &s = el.stream[i];
        if (s.mode != 1u) continue;
        uint32_t at = d.payload_offset[i] + ENTROPY_TABLE_BYTES + 4u * s.nblocks;   // (the container test has held the sizes to the payload)
        for (uint32_t b = 0; b < s.nblocks; b++) {
            const uint32_t size = codec_read<uint32_t>(bytes + s.payload_offset + ENTROPY_TABLE_BYTES + 4u * (size_t)b);
            table[2 * (d.st.first_block[i] + b)] = at;
            table[2 * (d.st.first_block[i] + b) + 1] = size;
            at += size;
        }
    }
    d.in = dev;
    d.block_at = (const uint32_t *)(dev + table_offset);
    d.channels = dev + upload_bytes;
    d.flags = (uint32_t *)(dev + upload_bytes + channel_bytes);
    d.occupancy = body;
    d.colours = (uint32_t *)(body + (l.colour_offset - l.occupancy_offset));
    d.tiles = body + (l.tile_offset - l.occupancy_offset);
    d.colour_words = codec_pad4(l.colour_bytes) / 4;
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 1);
    bool ok = hipMemcpyAsync(dev, host, table_offset + table_bytes, hipMemcpyHostToDevice, c.stream) == hipSuccess &&
              hipMemsetAsync(d.flags, 0, flag_bytes, c.stream) == hipSuccess;
    if (ok) {
        k::entropy_decode(d, report.device(), tag, c.stream);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;   // the one wait: the streams are in `body`, the check's word is here
    host_free(host, pinned);
    pool_free(dev);
    if (!ok || !report.landed(tag, 0)) {
        hip_failed(hipGetLastError(), "octree decode (entropy stage)", __FILE__, __LINE__);
        return false;
    }
    const uint32_t status = report.value(0);
    if (status & 1u) { note_error(who, "entropy-coded block is not intact"); return false; }
    if (status & 2u) { note_error(who, "occupancy byte is 0"); return false; }
    if (status & 4u) { note_error(who, "occupancy bits differ from the node count"); return false; }
    return true;
}

void fill_info(const CodecLayout &l, cwipc_hip_codec_info *info) {
    memset(info, 0, sizeof(*info));
    info->timestamp = l.timestamp;
    info->nleaves = l.nleaves;
    info->octree_bits = l.bits;
    info->colour_bits = l.colour_bits;
    info->tile_mode = l.tile_mode;
    info->tile_value = l.tile_value;
    for (int a = 0; a < 3; a++) info->min[a] = l.mn[a];
    info->side = l.side;
    for (int d = 0; d < l.bits; d++) info->nodes[d] = l.nodes[d];
    info->occupancy_offset = l.occupancy_offset;
    info->colour_offset = l.colour_offset;
    info->tile_offset = l.tile_offset;
    info->total_bytes = l.total_bytes;
}

// the caller-buffer convention of the two host conversions: the size of the result; its bytes are written iff they fit
size_t hand_out(const std::vector<uint8_t> &made, void *out, size_t capacity) {
    if (out != nullptr && made.size() <= capacity) memcpy(out, made.data(), made.size());
    return made.size();
}

// A frame of an inter-mode encoder: key or delta as the sequence rules and the device's answer say; the frame's leaves become the reference.
int encoder_feed_inter(const char *who, cwipc_hip_encoder *enc, const std::shared_ptr<DeviceSoA> &src, uint64_t timestamp) {
    std::lock_guard<std::mutex> guard(enc->inter_lock);
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const int bits = enc->params.octree_bits, shift = codec_colour_shift(enc->params.jpeg_quality);
    if (enc->reference) enc->reference->wait_on(c.stream);
    InterAsk ask;
    ask.allow_delta = !enc->sequence.at_gop_boundary();
    for (int a = 0; a < 3; a++) ask.gop_mn[a] = enc->gop_mn[a];
    ask.gop_side = enc->gop_side;
    ask.exp_factor = enc->params.exp_factor;
    Sorted s;
    std::unique_ptr<EncJob> job;
    std::unique_ptr<InterRefDev> next;
    if (sort_cloud(who, src, bits, s, &ask)) {
        CodecLayout l;
        emit_layout(s, bits, shift, timestamp, l);
        uint32_t gop_index = 0;
        const uint32_t kind = enc->sequence.next(l.nleaves == 0u, ask.delta, gop_index);
        bool ok = true;
        if (l.nleaves) {
            next = InterRefDev::make(l);
            if (!next) { note_error(who, "out of device memory"); ok = false; }
        }
        if (ok && kind == INTER_KEY) {
            job = emit_packet(who, s, bits, shift, timestamp, enc->entropy, INTER_PREFIX_BYTES, next ? &next->leaves : nullptr);
            if (job) {
                inter_write_prefix(job->host - INTER_PREFIX_BYTES, INTER_KEY, 0, 0, 0);
                if (l.nleaves) {
                    for (int a = 0; a < 3; a++) enc->gop_mn[a] = l.mn[a];
                    enc->gop_side = l.side;
                }
            }
        } else if (ok) {
            job = emit_delta(who, s, bits, shift, timestamp, gop_index, *enc->reference, next->leaves);
        }
        if (job && next && !next->published(c.stream)) {
            (void)c.sync();
            job.reset();
        }
        c.free_later(s.block);
    }
    if (!job) {   // the sequence starts anew with a key frame
        next.reset();
        enc->sequence = InterSequence();
        enc->sequence.gop_size = enc->params.gop_size;
    }
    replace_reference(enc->reference, std::move(next));
    if (!job) return -1;
    std::lock_guard<std::mutex> l(enc->lock);
    enc->queue.push_back(std::move(job));
    return 0;
}

int encoder_feed_sorted(const char *who, cwipc_hip_encoder *enc, const Sorted &s, uint64_t timestamp) {
    auto job = enc->transform ? emit_packet(who, s, enc->params.octree_bits, 0, timestamp, true, 0, nullptr, transform_q16(enc->params.jpeg_quality))
                              : emit_packet(who, s, enc->params.octree_bits, codec_colour_shift(enc->params.jpeg_quality), timestamp, enc->entropy);
    if (!job) return -1;
    std::lock_guard<std::mutex> l(enc->lock);
    enc->queue.push_back(std::move(job));
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------
// encoder
// ---------------------------------------------------------------------------
extern "C" cwipc_hip_encoder *cwipc_hip_new_encoder(const cwipc_hip_encoder_params *params, char **errorMessage) {
    const char *who = "cwipc_hip_new_encoder";
    ErrorbufScope scope(errorMessage);
    if (params == nullptr) { note_error(who, "NULL argument"); return nullptr; }
    if (const char *problem = params_problem(*params)) { note_error(who, problem); return nullptr; }
    cwipc_hip_encoder *enc = new (std::nothrow) cwipc_hip_encoder();
    if (!enc) { note_error(who, "out of memory"); return nullptr; }
    enc->params = *params;
    enc->inter = inter_params_on(params->do_inter_frame, params->gop_size, params->exp_factor);
    enc->sequence.gop_size = enc->inter ? params->gop_size : 1;
    return enc;
}

extern "C" void cwipc_hip_encoder_free(cwipc_hip_encoder *enc) {
    if (enc == nullptr || enc->in_group) return;   // (a group's encoders go with the group)
    delete enc;
}

extern "C" int cwipc_hip_encoder_feed(cwipc_hip_encoder *enc, cwipc_pointcloud *pc) {
    const char *who = "cwipc_hip_encoder_feed";
    return guarded(who, -1, [&]() -> int {
        if (enc == nullptr || pc == nullptr) { note_error(who, "NULL argument"); return -1; }
        if (enc->closed) { note_error(who, "the encoder has been closed"); return -1; }
        {
            std::lock_guard<std::mutex> l(enc->lock);
            enc->fed = true;
        }
        MadeClouds made;
        std::unique_ptr<cwipc_hip_pointcloud> keep;
        int rv = -1;
        auto src = filtered_input(who, pc, enc->params.tilenumber, enc->params.voxelsize, made.list, keep);
        if (src && enc->inter) {
            rv = encoder_feed_inter(who, enc, src, pc->timestamp());
        } else if (src) {
            Sorted s;
            if (sort_cloud(who, src, enc->params.octree_bits, s)) {
                rv = encoder_feed_sorted(who, enc, s, pc->timestamp());
                tctx().free_later(s.block);
            }
        }
        return rv;
    });
}

extern "C" int cwipc_hip_encoder_set_entropy(cwipc_hip_encoder *enc, int on) {
    const char *who = "cwipc_hip_encoder_set_entropy";
    if (enc == nullptr) { note_error(who, "NULL argument"); return -1; }
    std::lock_guard<std::mutex> l(enc->lock);
    if (enc->fed) { note_error(who, "the encoder has been fed: the packet form is chosen before the first feed"); return -1; }
    enc->entropy = on != 0;
    return 0;
}

extern "C" int cwipc_hip_encoder_set_colour_transform(cwipc_hip_encoder *enc, int on) {
    const char *who = "cwipc_hip_encoder_set_colour_transform";
    if (enc == nullptr) { note_error(who, "NULL argument"); return -1; }
    std::lock_guard<std::mutex> l(enc->lock);
    if (enc->fed) { note_error(who, "the encoder has been fed: the packet form is chosen before the first feed"); return -1; }
    if (on != 0 && enc->inter) {
        note_error(who, "inter mode: a delta's colour differences are exact residuals to the reference; transform colour under RULE P is out of scope");
        return -1;
    }
    enc->transform = on != 0;
    return 0;
}

extern "C" bool cwipc_hip_encoder_available(cwipc_hip_encoder *enc, bool wait) {
    if (enc == nullptr) return false;
    std::lock_guard<std::mutex> l(enc->lock);
    if (enc->queue.empty()) return false;
    return enc->queue.front()->ready(wait);
}

extern "C" size_t cwipc_hip_encoder_get_encoded_size(cwipc_hip_encoder *enc) {
    if (enc == nullptr) return 0;
    std::lock_guard<std::mutex> l(enc->lock);
    if (enc->queue.empty()) return 0;
    enc->queue.front()->finalize();
    return enc->queue.front()->packet_bytes();
}

extern "C" bool cwipc_hip_encoder_copy_data(cwipc_hip_encoder *enc, void *buffer, size_t size) {
    if (enc == nullptr || buffer == nullptr) return false;
    std::lock_guard<std::mutex> l(enc->lock);
    if (enc->queue.empty()) return false;
    EncJob &job = *enc->queue.front();
    job.finalize();
    if (size < job.packet_bytes()) return false;
    memcpy(buffer, job.host - job.prefix, job.packet_bytes());
    enc->queue.pop_front();
    return true;
}

extern "C" bool cwipc_hip_encoder_at_gop_boundary(cwipc_hip_encoder *enc) {
    if (enc == nullptr || !enc->inter) return true;
    std::lock_guard<std::mutex> guard(enc->inter_lock);
    return enc->sequence.at_gop_boundary();
}

extern "C" bool cwipc_hip_encoder_eof(cwipc_hip_encoder *enc) {
    if (enc == nullptr) return true;
    std::lock_guard<std::mutex> l(enc->lock);
    return enc->closed && enc->queue.empty();
}

extern "C" void cwipc_hip_encoder_close(cwipc_hip_encoder *enc) {
    if (enc == nullptr) return;
    std::lock_guard<std::mutex> l(enc->lock);
    enc->closed = true;
}

// ---------------------------------------------------------------------------
// encoder group
// ---------------------------------------------------------------------------
extern "C" cwipc_hip_encodergroup *cwipc_hip_new_encodergroup(char **errorMessage) {
    ErrorbufScope scope(errorMessage);
    cwipc_hip_encodergroup *g = new (std::nothrow) cwipc_hip_encodergroup();
    if (!g) note_error("cwipc_hip_new_encodergroup", "out of memory");
    return g;
}

extern "C" cwipc_hip_encoder *cwipc_hip_encodergroup_addencoder(cwipc_hip_encodergroup *group, const cwipc_hip_encoder_params *params, char **errorMessage) {
    if (group == nullptr) {
        ErrorbufScope scope(errorMessage);
        note_error("cwipc_hip_encodergroup_addencoder", "NULL argument");
        return nullptr;
    }
    if (params != nullptr && inter_params_on(params->do_inter_frame, params->gop_size, params->exp_factor)) {
        ErrorbufScope scope(errorMessage);
        note_error("cwipc_hip_encodergroup_addencoder", "do_inter_frame: inter-frame coding is not available inside an encoder group (out of scope)");
        return nullptr;
    }
    cwipc_hip_encoder *enc = cwipc_hip_new_encoder(params, errorMessage);
    if (!enc) return nullptr;
    enc->in_group = true;
    std::lock_guard<std::mutex> l(group->lock);
    try {
        group->encoders.push_back(enc);
    } catch (...) {
        delete enc;
        ErrorbufScope scope(errorMessage);
        note_error("cwipc_hip_encodergroup_addencoder", "out of memory");
        return nullptr;
    }
    return enc;
}

extern "C" int cwipc_hip_encodergroup_feed(cwipc_hip_encodergroup *group, cwipc_pointcloud *pc) {
    const char *who = "cwipc_hip_encodergroup_feed";
    return guarded(who, -1, [&]() -> int {
        if (group == nullptr || pc == nullptr) { note_error(who, "NULL argument"); return -1; }
        std::lock_guard<std::mutex> l(group->lock);
        // the encoders that work on the same cloud, in the order of their first member
        std::vector<std::vector<cwipc_hip_encoder *>> classes;
        for (cwipc_hip_encoder *enc : group->encoders) {
            if (enc->closed) continue;
            {
                std::lock_guard<std::mutex> el(enc->lock);
                enc->fed = true;
            }
            bool placed = false;
            for (auto &cls : classes)
                if (cls[0]->params.tilenumber == enc->params.tilenumber && cls[0]->params.voxelsize == enc->params.voxelsize) { cls.push_back(enc); placed = true; break; }
            if (!placed) classes.push_back({enc});
        }
        int rv = 0;
        for (auto &cls : classes) {
            MadeClouds made;
            std::unique_ptr<cwipc_hip_pointcloud> keep;
            int bits = 0;
            for (cwipc_hip_encoder *enc : cls) bits = enc->params.octree_bits > bits ? enc->params.octree_bits : bits;
            auto src = filtered_input(who, pc, cls[0]->params.tilenumber, cls[0]->params.voxelsize, made.list, keep);
            Sorted s;
            if (src && sort_cloud(who, src, bits, s)) {
                for (cwipc_hip_encoder *enc : cls)
                    if (encoder_feed_sorted(who, enc, s, pc->timestamp()) != 0) rv = -1;
                tctx().free_later(s.block);
            } else {
                rv = -1;
            }
        }
        return rv;
    });
}

extern "C" void cwipc_hip_encodergroup_close(cwipc_hip_encodergroup *group) {
    if (group == nullptr) return;
    std::lock_guard<std::mutex> l(group->lock);
    for (cwipc_hip_encoder *enc : group->encoders) cwipc_hip_encoder_close(enc);
}

extern "C" void cwipc_hip_encodergroup_free(cwipc_hip_encodergroup *group) {
    if (group == nullptr) return;
    for (cwipc_hip_encoder *enc : group->encoders) delete enc;
    delete group;
}

// ---------------------------------------------------------------------------
// decoder
// ---------------------------------------------------------------------------
extern "C" int cwipc_hip_codec_packet_info(const void *bytes, size_t len, cwipc_hip_codec_info *info, char **errorMessage) {
    const char *who = "cwipc_hip_codec_packet_info";
    ErrorbufScope scope(errorMessage);
    CodecLayout l;
    if (const char *problem = codec_validate((const uint8_t *)bytes, len, l)) { note_error(who, problem); return -1; }
    if (info) fill_info(l, info);
    return 0;
}

// ---------------------------------------------------------------------------
// the entropy-coded form on the host (no GPU)
// ---------------------------------------------------------------------------
extern "C" size_t cwipc_hip_codec_entropy_pack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage) {
    const char *who = "cwipc_hip_codec_entropy_pack";
    ErrorbufScope scope(errorMessage);
    return guarded(who, (size_t)0, [&]() -> size_t {
        std::vector<uint8_t> made;
        if (const char *problem = entropy_pack((const uint8_t *)bytes, len, made)) { note_error(who, problem); return 0; }
        return hand_out(made, out, capacity);
    });
}

extern "C" size_t cwipc_hip_codec_entropy_unpack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage) {
    const char *who = "cwipc_hip_codec_entropy_unpack";
    ErrorbufScope scope(errorMessage);
    return guarded(who, (size_t)0, [&]() -> size_t {
        std::vector<uint8_t> made;
        if (const char *problem = entropy_unpack((const uint8_t *)bytes, len, made)) { note_error(who, problem); return 0; }
        return hand_out(made, out, capacity);
    });
}

extern "C" int cwipc_hip_codec_entropy_info(const void *bytes, size_t len, cwipc_hip_codec_entropy_directory *info, char **errorMessage) {
    const char *who = "cwipc_hip_codec_entropy_info";
    ErrorbufScope scope(errorMessage);
    EntropyLayout e;
    if (const char *problem = entropy_validate((const uint8_t *)bytes, len, e)) { note_error(who, problem); return -1; }
    if (info) {
        memset(info, 0, sizeof(*info));
        fill_info(e.cwao, &info->packet);
        info->nstreams = e.nstreams;
        for (int i = 0; i < e.nstreams; i++) {
            info->kind[i] = (int32_t)e.stream[i].kind;
            info->which[i] = (int32_t)e.stream[i].which;
            info->mode[i] = (int32_t)e.stream[i].mode;
            info->symbols[i] = e.stream[i].symbols;
            info->payload_offset[i] = e.stream[i].payload_offset;
            info->payload_bytes[i] = e.stream[i].payload_bytes;
        }
        info->total_bytes = e.total_bytes;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// transform colour coding on the host (no GPU)
// ---------------------------------------------------------------------------
extern "C" size_t cwipc_hip_codec_transform_pack(const void *bytes, size_t len, int jpeg_quality, void *out, size_t capacity, char **errorMessage) {
    const char *who = "cwipc_hip_codec_transform_pack";
    ErrorbufScope scope(errorMessage);
    return guarded(who, (size_t)0, [&]() -> size_t {
        std::vector<uint8_t> made;
        if (const char *problem = transform_pack((const uint8_t *)bytes, len, jpeg_quality, made)) { note_error(who, problem); return 0; }
        return hand_out(made, out, capacity);
    });
}

extern "C" size_t cwipc_hip_codec_transform_unpack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage) {
    const char *who = "cwipc_hip_codec_transform_unpack";
    ErrorbufScope scope(errorMessage);
    return guarded(who, (size_t)0, [&]() -> size_t {
        std::vector<uint8_t> made;
        if (const char *problem = transform_unpack((const uint8_t *)bytes, len, made)) { note_error(who, problem); return 0; }
        return hand_out(made, out, capacity);
    });
}

extern "C" int cwipc_hip_codec_transform_info(const void *bytes, size_t len, cwipc_hip_codec_transform_directory *info, char **errorMessage) {
    const char *who = "cwipc_hip_codec_transform_info";
    ErrorbufScope scope(errorMessage);
    TransformLayout t;
    if (const char *problem = transform_validate((const uint8_t *)bytes, len, t)) { note_error(who, problem); return -1; }
    if (info) {
        memset(info, 0, sizeof(*info));
        fill_info(t.cwao, &info->packet);
        info->q16 = t.q16;
        for (int ch = 0; ch < 3; ch++) {
            info->dc[ch] = t.dc[ch];
            info->nescapes[ch] = t.nescapes[ch];
        }
        info->nstreams = t.nstreams;
        for (int i = 0; i < t.nstreams; i++) {
            info->kind[i] = (int32_t)t.stream[i].kind;
            info->which[i] = (int32_t)t.stream[i].which;
            info->mode[i] = (int32_t)t.stream[i].mode;
            info->symbols[i] = t.stream[i].symbols;
            info->payload_offset[i] = t.stream[i].payload_offset;
            info->payload_bytes[i] = t.stream[i].payload_bytes;
        }
        info->total_bytes = t.total_bytes;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// inter-frame packets on the host (no GPU)
// ---------------------------------------------------------------------------
extern "C" size_t cwipc_hip_codec_inter_pack(const void *r, size_t rlen, const void *p, size_t plen, uint32_t gop_index, void *out, size_t capacity,
                                             char **errorMessage) {
    const char *who = "cwipc_hip_codec_inter_pack";
    ErrorbufScope scope(errorMessage);
    return guarded(who, (size_t)0, [&]() -> size_t {
        std::vector<uint8_t> made;
        if (const char *problem = inter_pack((const uint8_t *)r, rlen, (const uint8_t *)p, plen, gop_index, made)) { note_error(who, problem); return 0; }
        return hand_out(made, out, capacity);
    });
}

extern "C" size_t cwipc_hip_codec_inter_unpack(const void *r, size_t rlen, const void *d, size_t dlen, void *out, size_t capacity, char **errorMessage) {
    const char *who = "cwipc_hip_codec_inter_unpack";
    ErrorbufScope scope(errorMessage);
    return guarded(who, (size_t)0, [&]() -> size_t {
        std::vector<uint8_t> made;
        if (const char *problem = inter_unpack((const uint8_t *)r, rlen, (const uint8_t *)d, dlen, made)) { note_error(who, problem); return 0; }
        return hand_out(made, out, capacity);
    });
}

extern "C" int cwipc_hip_codec_inter_info(const void *bytes, size_t len, cwipc_hip_codec_inter_directory *info, char **errorMessage) {
    const char *who = "cwipc_hip_codec_inter_info";
    ErrorbufScope scope(errorMessage);
    InterLayout e;
    if (const char *problem = inter_validate((const uint8_t *)bytes, len, nullptr, e)) { note_error(who, problem); return -1; }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->kind = e.kind;
        info->gop_index = e.gop_index;
        info->ref_timestamp = e.ref_timestamp;
        info->ref_nleaves = e.ref_nleaves;
        info->embedded_entropy = e.embedded_entropy ? 1 : 0;
        fill_info(e.cwao, &info->packet);
        info->nadded = e.nadded;
        for (int d = 0; d < e.cwao.bits; d++) info->nodes_added[d] = e.nodes_added[d];
        info->nstreams = e.nstreams;
        for (int i = 0; i < e.nstreams; i++) {
            info->kind_of[i] = (int32_t)e.stream[i].kind;
            info->which[i] = (int32_t)e.stream[i].which;
            info->mode[i] = (int32_t)e.stream[i].mode;
            info->symbols[i] = e.stream[i].symbols;
            info->payload_offset[i] = e.stream[i].payload_offset;
            info->payload_bytes[i] = e.stream[i].payload_bytes;
        }
        info->total_bytes = e.total_bytes;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// level-of-detail cuts of packets on the host (no GPU)
// ---------------------------------------------------------------------------
extern "C" size_t cwipc_hip_codec_lod(const void *bytes, size_t len, int bits, void *out, size_t capacity, char **errorMessage) {
    const char *who = "cwipc_hip_codec_lod";
    ErrorbufScope scope(errorMessage);
    return guarded(who, (size_t)0, [&]() -> size_t {
        std::vector<uint8_t> made;
        if (const char *problem = lod_convert((const uint8_t *)bytes, len, bits, made)) { note_error(who, problem); return 0; }
        return hand_out(made, out, capacity);
    });
}

extern "C" cwipc_hip_decoder *cwipc_hip_new_decoder(char **errorMessage) {
    ErrorbufScope scope(errorMessage);
    cwipc_hip_decoder *d = new (std::nothrow) cwipc_hip_decoder();
    if (!d) note_error("cwipc_hip_new_decoder", "out of memory");
    return d;
}

namespace {

// A "cwao" or "cwae" packet into a cloud on the decoder's queue.  keep_reference (the packet is a key packet's, RULE P; the caller
// holds the decoder's inter_lock): the frame's leaves become the decoder's reference, none for an empty cloud.
// max_bits (RULE L): a packet of more bits gives the cloud of its cut; the reference is the full frame all the same.
int decoder_feed_plain(const char *who, cwipc_hip_decoder *dec, const void *bytes, size_t len, bool keep_reference, int max_bits) {
    // the validity test: host code, before anything is launched or allocated on the device
    CodecLayout l;
    EntropyLayout el;
    const bool coded = bytes != nullptr && len >= 4 && codec_read<uint32_t>((const uint8_t *)bytes) == ENTROPY_MAGIC;
    if (const char *problem = coded ? entropy_validate((const uint8_t *)bytes, len, el) : codec_validate((const uint8_t *)bytes, len, l)) {
        note_error(who, problem);
        return -1;
    }
    if (coded) {
        l = el.cwao;
        if (el.total_bytes > 0x7fffffffull) { note_error(who, "the packet is too large"); return -1; }
    }
    if (!device_available(who)) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const int out_bits = lod_out_bits(l.bits, max_bits);
    const bool cut = out_bits < l.bits && l.nleaves;
    const double cell = codec_cellsize(l.side, out_bits);
    cwipc_hip_decoder::Job job;
    std::shared_ptr<DeviceSoA> dst;   // (the cut of a key packet's frame is made from the reference's leaves, below)
    if (!(cut && keep_reference)) {
        dst = soa_alloc(cut ? l.nodes[out_bits - 1] : l.nleaves);
        if (!dst) { note_error(who, "out of device memory"); return -1; }
    }
    if (l.nleaves) {
        const size_t body = (size_t)(l.total_bytes - l.occupancy_offset);
        k::CodecDecode d{};
        d.bits = l.bits;
        d.colour_bits = l.colour_bits;
        d.tile_value = l.tile_value;
        d.nleaves = l.nleaves;
        for (int i = 0; i < l.bits; i++) d.nodes[i] = l.nodes[i];
        for (int a = 0; a < 3; a++) d.mn[a] = l.mn[a];
        d.cell = cell;
        d.colour_words = codec_pad4(l.colour_bytes) / 4;
        const size_t body_bytes = round256(body + 8), ping_bytes = round256((size_t)l.nleaves * 8), scratch_bytes = round256(k::codec_decode_scratch_words(d) * 4);
        uint8_t *block = (uint8_t *)pool_alloc(body_bytes + 2 * ping_bytes + scratch_bytes);
        if (!coded) job.host = (uint8_t *)host_alloc(body, &job.pinned);
        if (!block || (!coded && !job.host)) {
            pool_free(block);
            if (job.host) host_free(job.host, job.pinned);
            note_error(who, "out of memory");
            return -1;
        }
        d.colours = (const uint32_t *)(block + (l.colour_offset - l.occupancy_offset));
        d.tiles = l.tile_mode == 1 ? block + (l.tile_offset - l.occupancy_offset) : nullptr;
        bool ok = true;
        if (coded) {
            // the body comes from the entropy stage; a packet it refuses ends here, before any kernel of the octree decoder
            if (!entropy_to_body(who, c, (const uint8_t *)bytes, el, block)) {
                pool_free(block);
                return -1;
            }
        } else {
            memcpy(job.host, (const uint8_t *)bytes + l.occupancy_offset, body);
            ok = hipMemcpyAsync(block, job.host, body, hipMemcpyHostToDevice, c.stream) == hipSuccess;
        }
        if (ok) {
            unsigned long long *ping = (unsigned long long *)(block + body_bytes), *pong = (unsigned long long *)(block + body_bytes + ping_bytes);
            uint32_t *scratch = (uint32_t *)(block + body_bytes + 2 * ping_bytes);
            if (!cut) k::codec_decode(block, d, ping, pong, scratch, *dst, c.stream);
            else if (keep_reference) (void)k::codec_expand(block, d, ping, pong, scratch, c.stream);   // the full keys, for the reference
            else ok = lod_from_body(who, c, block, l, d, out_bits, nullptr, *dst);
            ok = ok && hipGetLastError() == hipSuccess;
        }
        c.free_later(block);
        if (!ok) {
            (void)c.sync();
            if (job.host) host_free(job.host, job.pinned);
            hip_failed(hipGetLastError(), "octree decode", __FILE__, __LINE__);
            return -1;
        }
        if (keep_reference) {
            // the leaves as the kernels above left them: the keys where the last depth's expansion wrote them
            std::unique_ptr<InterRefDev> next = InterRefDev::make(l);
            const uint8_t *leaf_keys = block + body_bytes + (l.bits % 2 ? ping_bytes : 0);
            if (!next || hipMemcpyAsync(next->leaves.keys, leaf_keys, 8u * (size_t)l.nleaves, hipMemcpyDeviceToDevice, c.stream) != hipSuccess) {
                (void)c.sync();
                if (job.host) host_free(job.host, job.pinned);
                note_error(who, "the reference could not be kept");
                return -1;
            }
            k::inter_leaves_of_planes(d.colours, d.colour_words, d.tiles, d.tile_value, l.colour_bits, next->leaves, c.stream);
            if (!next->published(c.stream)) (void)c.sync();
            replace_reference(dec->reference, std::move(next));
            if (cut) {
                dst = lod_from_leaves(who, c, dec->reference->leaves, l, out_bits);
                if (!dst) {
                    if (job.host) host_free(job.host, job.pinned);
                    return -1;
                }
            }
        }
        dst->mark_pending(c.stream);
    } else if (keep_reference) {
        replace_reference(dec->reference, nullptr);
    }
    auto *cloud = new cwipc_hip_pointcloud();
    cloud->adopt_device(dst, l.timestamp, (float)cell);
    job.cloud = cloud;
    job.planes = dst;
    std::lock_guard<std::mutex> lk(dec->lock);
    dec->queue.push_back(job);
    return 0;
}

// A "cwat" packet (RULE T) into a cloud on the decoder's queue: the container test on the host -> upload -> the streams decoded
// (occupancy and tiles into the body the octree decoder reads, the tokens into byte planes), the tree's first children, the tokens and
// escapes joined -> ONE wait for the entropy stage's status and the three counts of tokens equal to 255 (a packet that fails is refused
// there) -> weights, the inverse transform into the body's colour plane, the octree decoder.
int decoder_feed_transform(const char *who, cwipc_hip_decoder *dec, const uint8_t *bytes, size_t len, int max_bits) {
    TransformLayout tl;
    if (const char *problem = transform_validate(bytes, len, tl)) { note_error(who, problem); return -1; }
    const CodecLayout &l = tl.cwao;
    if (tl.total_bytes > 0x7fffffffull || (uint64_t)l.occupancy_bytes + l.nleaves > 0x7fffffffull) { note_error(who, "the packet is too large"); return -1; }
    if (!device_available(who)) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const int out_bits = lod_out_bits(l.bits, max_bits);
    const bool cut = out_bits < l.bits && l.nleaves;   // RULE L on the 8-colour-bit packet this one stands for: the inverse transform runs in full
    const double cell = codec_cellsize(l.side, out_bits);
    auto dst = soa_alloc(cut ? l.nodes[out_bits - 1] : l.nleaves);
    if (!dst) { note_error(who, "out of device memory"); return -1; }
    if (l.nleaves) {
        const size_t n = l.nleaves, ncoef = n - 1, body = (size_t)(l.total_bytes - l.occupancy_offset);
        k::CodecDecode cd{};
        cd.bits = l.bits;
        cd.colour_bits = 8;
        cd.tile_value = l.tile_value;
        cd.nleaves = l.nleaves;
        for (int i = 0; i < l.bits; i++) cd.nodes[i] = l.nodes[i];
        for (int a = 0; a < 3; a++) cd.mn[a] = l.mn[a];
        cd.cell = cell;
        cd.colour_words = codec_pad4(l.colour_bytes) / 4;
        // the entropy stage's streams: every stream but the escapes, which the transform's kernels read where the upload put them
        k::EntropyDecode d{};
        uint32_t escape_offset[3] = {0, 0, 0};
        d.st.colour_bits = 8;
        d.st.nleaves = l.nleaves;
        int stream_of[ENTROPY_MAX_STREAMS];
        for (int i = 0; i < tl.nstreams; i++) {
            const EntropyStream &s = tl.stream[i];
            if (s.kind == TRANSFORM_ESCAPE) { escape_offset[s.which] = (uint32_t)(s.payload_offset - tl.directory_offset); continue; }
            const int j = d.st.nstreams++;
            stream_of[j] = i;
            d.st.kind[j] = s.kind;
            d.st.which[j] = s.which;
            d.st.symbols[j] = s.symbols;
            d.st.first_block[j] = d.st.total_blocks;
            d.st.total_blocks += s.nblocks;
            d.st.plane_offset[j] = s.kind == ENTROPY_OCCUPANCY ? (uint32_t)entropy_depth_offset(l, (int)s.which) : s.kind == ENTROPY_BYTES ? (uint32_t)(s.which * ncoef) : 0u;
            d.st.raw_padded[j] = (uint32_t)codec_pad4(s.raw_bytes);
            d.mode[j] = s.mode;
            d.payload_offset[j] = (uint32_t)(s.payload_offset - tl.directory_offset);
            d.payload_bytes[j] = (uint32_t)s.payload_bytes;
            d.children[j] = s.kind == ENTROPY_OCCUPANCY ? l.nodes[s.which] : 0u;
        }
        k::TransformTree tree{};
        k::transform_tree_counts(tree, l.bits, l.nodes, l.nleaves, tl.q16);
        const size_t inner = tree.inner, total = inner + n;
        const size_t body_bytes = round256(body + 8), ping_bytes = round256(n * 8), scratch_bytes = round256(k::codec_decode_scratch_words(cd) * 4);
        const size_t in_bytes = (size_t)(tl.total_bytes - tl.directory_offset), table_offset = (in_bytes + 7) & ~(size_t)7, table_bytes = 8u * (size_t)d.st.total_blocks,
                     upload_bytes = round256(table_offset + table_bytes), flag_bytes = round256(4u * (size_t)(1 + d.st.nstreams));
        const size_t first_at = 0, weight_at = first_at + round256(4 * inner), value_at = weight_at + round256(4 * inner), zz_at = value_at + round256(12 * total),
                     scan_at = zz_at + round256(12 * ncoef + 4), tokens_at = scan_at + round256(4 * k::transform_scan_words(tree)),
                     tree_bytes = tokens_at + round256(3 * ncoef + 4);
        bool pinned = false;
        uint8_t *host = (uint8_t *)host_alloc(upload_bytes, &pinned);
        uint8_t *block = (uint8_t *)pool_alloc(body_bytes + 2 * ping_bytes + scratch_bytes);
        uint8_t *dev = (uint8_t *)pool_alloc(upload_bytes + flag_bytes);
        uint8_t *tblock = (uint8_t *)pool_alloc(tree_bytes);
        auto give_back = [&]() {
            if (host) host_free(host, pinned);
            pool_free(block);
            pool_free(dev);
            pool_free(tblock);
        };
        if (!host || !block || !dev || !tblock) {
            give_back();
            note_error(who, "out of memory");
            return -1;
        }
        memcpy(host, bytes + tl.directory_offset, in_bytes);
        uint32_t *table = (uint32_t *)(host + table_offset);
        memset(table, 0, table_bytes);
        for (int j = 0; j < d.st.nstreams; j++) {
            const EntropyStream &s = tl.stream[stream_of[j]];
            if (s.mode != 1u) continue;
            uint32_t at = d.payload_offset[j] + ENTROPY_TABLE_BYTES + 4u * s.nblocks;   // (the container test has held the sizes to the payload)
            for (uint32_t b = 0; b < s.nblocks; b++) {
                const uint32_t size = codec_read<uint32_t>(bytes + s.payload_offset + ENTROPY_TABLE_BYTES + 4u * (size_t)b);
                table[2 * (d.st.first_block[j] + b)] = at;
                table[2 * (d.st.first_block[j] + b) + 1] = size;
                at += size;
            }
        }
        uint8_t *colours = block + (l.colour_offset - l.occupancy_offset);
        d.in = dev;
        d.block_at = (const uint32_t *)(dev + table_offset);
        d.planes = tblock + tokens_at;
        d.flags = (uint32_t *)(dev + upload_bytes);
        d.occupancy = block;
        d.tiles = block + (l.tile_offset - l.occupancy_offset);
        tree.occupancy = block;
        tree.first = (uint32_t *)(tblock + first_at);
        tree.weight = (uint32_t *)(tblock + weight_at);
        tree.value = (int32_t *)(tblock + value_at);
        tree.zz = (uint32_t *)(tblock + zz_at);
        tree.scan = (uint32_t *)(tblock + scan_at);
        PinnedReport report = c.report();
        const uint32_t tag = report.arm(0, 4);   // word 0: the entropy stage's status; words 1 .. 3: the tokens equal to 255 of Y, Co, Cg
        bool ok = hipMemcpyAsync(dev, host, table_offset + table_bytes, hipMemcpyHostToDevice, c.stream) == hipSuccess &&
                  hipMemsetAsync(d.flags, 0, flag_bytes, c.stream) == hipSuccess;
        if (ok) {
            k::entropy_decode(d, report.device(), tag, c.stream);
            k::transform_prepare(tree, c.stream);
            k::transform_untoken(tree, d.planes, dev, escape_offset, tl.nescapes, report.device() + 1, tag, c.stream);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = c.sync() && ok;   // the one wait
        host_free(host, pinned);
        host = nullptr;
        if (!ok || !report.landed(tag, 0, 4)) {
            give_back();
            hip_failed(hipGetLastError(), "octree decode (transform stage)", __FILE__, __LINE__);
            return -1;
        }
        const uint32_t status = report.value(0);
        const char *problem = status & 1u   ? "entropy-coded block is not intact"
                              : status & 2u ? "occupancy byte is 0"
                              : status & 4u ? "occupancy bits differ from the node count"
                                            : nullptr;
        for (int ch = 0; ch < 3 && !problem; ch++)
            if (report.value(1 + ch) != tl.nescapes[ch]) problem = "tokens equal to 255 differ from the escape count";
        if (problem) {
            give_back();
            note_error(who, problem);
            return -1;
        }
        cd.colours = (const uint32_t *)colours;
        cd.tiles = l.tile_mode == 1 ? d.tiles : nullptr;
        k::transform_inverse(tree, tl.dc, colours, c.stream);
        if (cut) ok = lod_from_body(who, c, block, l, cd, out_bits, tree.first, *dst);
        else k::codec_decode(block, cd, (unsigned long long *)(block + body_bytes), (unsigned long long *)(block + body_bytes + ping_bytes),
                             (uint32_t *)(block + body_bytes + 2 * ping_bytes), *dst, c.stream);
        ok = ok && hipGetLastError() == hipSuccess;
        c.free_later(block);
        c.free_later(dev);
        c.free_later(tblock);
        if (!ok) {
            (void)c.sync();
            hip_failed(hipGetLastError(), "octree decode", __FILE__, __LINE__);
            return -1;
        }
        dst->mark_pending(c.stream);
    }
    cwipc_hip_decoder::Job job;
    auto *cloud = new cwipc_hip_pointcloud();
    cloud->adopt_device(dst, l.timestamp, (float)cell);
    job.cloud = cloud;
    job.planes = dst;
    std::lock_guard<std::mutex> lk(dec->lock);
    dec->queue.push_back(job);
    return 0;
}

// A delta packet (RULE P) that has passed inter_validate() against the reference held (the caller holds the decoder's inter_lock):
// upload, the streams decoded into byte planes, the added keys expanded, the checks, ONE wait; a delta that fails a check ends there,
// with the reference as it was.  Then the merge, the colours and tiles, the points; the frame becomes the reference.
int decoder_feed_delta(const char *who, cwipc_hip_decoder *dec, const uint8_t *bytes, const InterLayout &il, int max_bits) {
    if (!device_available(who)) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const CodecLayout &l = il.cwao;
    const InterRefDev &R = *dec->reference;
    const size_t n = l.nleaves, nr = R.leaves.n, nadded = il.nadded;
    const size_t keep_bytes = (nr + 7) / 8, res_offset = round256(keep_bytes), planes_bytes = res_offset + round256(4 * n);
    k::EntropyDecode d{};
    d.st.nstreams = il.nstreams;
    d.st.colour_bits = l.colour_bits;
    d.st.nleaves = l.nleaves;
    for (int i = 0; i < il.nstreams; i++) {
        const EntropyStream &es = il.stream[i];
        d.st.kind[i] = es.kind;
        d.st.which[i] = es.which;
        d.st.symbols[i] = es.symbols;
        d.st.first_block[i] = d.st.total_blocks;
        d.st.total_blocks += es.nblocks;
        d.st.plane_offset[i] = es.kind == ENTROPY_OCCUPANCY ? (uint32_t)inter_depth_offset(il.nodes_added, (int)es.which)
                               : es.kind == ENTROPY_BITS    ? (uint32_t)(res_offset + (size_t)es.which * n)
                               : es.which == 1u             ? (uint32_t)(res_offset + 3 * n)
                                                            : 0u;
        d.st.raw_padded[i] = (uint32_t)codec_pad4(es.raw_bytes);
        d.mode[i] = es.mode;
        d.payload_offset[i] = (uint32_t)(es.payload_offset - il.directory_offset);
        d.payload_bytes[i] = (uint32_t)es.payload_bytes;
        d.children[i] = es.children;
    }
    k::CodecDecode added_tree{};   // the tree of the added leaves, for codec_expand
    added_tree.bits = l.bits;
    added_tree.nleaves = il.nadded;
    for (int i = 0; i < l.bits; i++) added_tree.nodes[i] = il.nodes_added[i];
    const uint64_t occupancy_bytes = nadded ? inter_depth_offset(il.nodes_added, l.bits - 1) + (l.bits > 1 ? il.nodes_added[l.bits - 2] : 1u) : 0u;
    const size_t in_bytes = (size_t)(il.total_bytes - il.directory_offset), table_offset = (in_bytes + 7) & ~(size_t)7,
                 table_bytes = 8u * (size_t)d.st.total_blocks, upload_bytes = round256(table_offset + table_bytes),
                 occupancy_block = round256((size_t)occupancy_bytes + 8), ping_bytes = round256(8 * nadded + 8),
                 scratch_bytes = round256(k::codec_decode_scratch_words(added_tree) * 4), nrb = k::codec_blocks(nr),
                 rank_bytes = round256((nr + 1) * 4), counts_bytes = round256((nrb + 1) * 4), flag_bytes = 256;
    const size_t planes_at = upload_bytes, occupancy_at = planes_at + planes_bytes, ping_at = occupancy_at + occupancy_block, scratch_at = ping_at + 2 * ping_bytes,
                 rank_at = scratch_at + scratch_bytes, counts_at = rank_at + rank_bytes, flags_at = counts_at + counts_bytes;
    bool pinned = false;
    uint8_t *host = (uint8_t *)host_alloc(upload_bytes, &pinned);
    uint8_t *dev = (uint8_t *)pool_alloc(flags_at + flag_bytes);
    if (!host || !dev) {
        if (host) host_free(host, pinned);
        pool_free(dev);
        note_error(who, "out of memory");
        return -1;
    }
    memcpy(host, bytes + il.directory_offset, in_bytes);
    uint32_t *table = (uint32_t *)(host + table_offset);
    memset(table, 0, table_bytes);
    for (int i = 0; i < il.nstreams; i++) {
        const EntropyStream &es = il.stream[i];
        if (es.mode != 1u) continue;
        uint32_t at = d.payload_offset[i] + ENTROPY_TABLE_BYTES + 4u * es.nblocks;   // (the container test has held the sizes to the payload)
        for (uint32_t b = 0; b < es.nblocks; b++) {
            const uint32_t size = codec_read<uint32_t>(bytes + es.payload_offset + ENTROPY_TABLE_BYTES + 4u * (size_t)b);
            table[2 * (d.st.first_block[i] + b)] = at;
            table[2 * (d.st.first_block[i] + b) + 1] = size;
            at += size;
        }
    }
    d.in = dev;
    d.block_at = (const uint32_t *)(dev + table_offset);
    d.planes = dev + planes_at;
    d.occupancy = dev + occupancy_at;
    d.flags = (uint32_t *)(dev + flags_at);   // words 0 .. S: the entropy stage's; word 32: the checks'
    const uint8_t *keep = d.planes, *res = d.planes + res_offset;
    unsigned long long *ping = (unsigned long long *)(dev + ping_at), *pong = (unsigned long long *)(dev + ping_at + ping_bytes);
    uint32_t *rank = (uint32_t *)(dev + rank_at);
    R.wait_on(c.stream);
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 3);   // word 0: the entropy stage's status; word 1: the checks'; word 2: the kept leaves
    bool ok = hipMemcpyAsync(dev, host, table_offset + table_bytes, hipMemcpyHostToDevice, c.stream) == hipSuccess &&
              hipMemsetAsync(d.flags, 0, flag_bytes, c.stream) == hipSuccess;
    const unsigned long long *added = ping;
    if (ok) {
        k::entropy_decode(d, report.device(), tag, c.stream);
        if (nadded) added = k::codec_expand(d.occupancy, added_tree, ping, pong, (uint32_t *)(dev + scratch_at), c.stream);
        k::inter_check(R.leaves, keep, added, il.nadded, l.nleaves, rank, (uint32_t *)(dev + counts_at), d.flags + 32, report.device() + 1, tag, c.stream);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;   // the one wait: the streams are in their planes, the two status words are here
    host_free(host, pinned);
    if (!ok || !report.landed(tag, 0) || !report.landed(tag, 1)) {
        pool_free(dev);
        hip_failed(hipGetLastError(), "octree decode (delta)", __FILE__, __LINE__);
        return -1;
    }
    const uint32_t status = report.value(0) | report.value(1);
    const char *problem = status & 1u    ? "entropy-coded block is not intact"
                          : status & 2u  ? "occupancy byte is 0"
                          : status & 4u  ? "occupancy bits differ from the node count"
                          : status & 16u ? "padding bits of the kept leaves are not 0"
                          : status & 32u ? "kept and added leaves differ from the leaf count"
                          : status & 8u  ? "an added leaf is a leaf of the reference"
                                         : nullptr;
    if (problem) {
        pool_free(dev);
        note_error(who, problem);
        return -1;
    }
    const double cell = codec_cellsize(l.side, l.bits);
    auto dst = soa_alloc(l.nleaves);
    std::unique_ptr<InterRefDev> next = InterRefDev::make(l);
    if (!dst || !next) {
        pool_free(dev);
        note_error(who, "out of device memory");
        return -1;
    }
    k::CodecDecode points{};
    points.bits = l.bits;
    points.colour_bits = l.colour_bits;
    points.tile_value = l.tile_value;
    points.nleaves = l.nleaves;
    for (int a = 0; a < 3; a++) points.mn[a] = l.mn[a];
    points.cell = cell;
    k::inter_apply(R.leaves, keep, rank, added, il.nadded, res, points, l.tile_mode, next->leaves, *dst, c.stream);
    ok = hipGetLastError() == hipSuccess && next->published(c.stream);
    c.free_later(dev);
    if (!ok) {
        (void)c.sync();
        hip_failed(hipGetLastError(), "octree decode (delta)", __FILE__, __LINE__);
        return -1;
    }
    replace_reference(dec->reference, std::move(next));
    // RULE L: the reference stays the full frame, so the chain does not drift; only the cloud handed out is cut, from the frame's leaves
    const int out_bits = lod_out_bits(l.bits, max_bits);
    if (out_bits < l.bits && l.nleaves) {
        dst = lod_from_leaves(who, c, dec->reference->leaves, l, out_bits);
        if (!dst) return -1;
    }
    dst->mark_pending(c.stream);
    cwipc_hip_decoder::Job job;
    auto *cloud = new cwipc_hip_pointcloud();
    cloud->adopt_device(dst, l.timestamp, (float)codec_cellsize(l.side, out_bits));
    job.cloud = cloud;
    job.planes = dst;
    std::lock_guard<std::mutex> lk(dec->lock);
    dec->queue.push_back(job);
    return 0;
}
}  // namespace

extern "C" int cwipc_hip_decoder_feed(cwipc_hip_decoder *dec, const void *bytes, size_t len) {
    const char *who = "cwipc_hip_decoder_feed";
    return guarded(who, -1, [&]() -> int {
        if (dec == nullptr) { note_error(who, "NULL argument"); return -1; }
        if (dec->closed) { note_error(who, "the decoder has been closed"); return -1; }
        const int max_bits = dec->max_bits.load();
        if (bytes != nullptr && len >= 4 && codec_read<uint32_t>((const uint8_t *)bytes) == TRANSFORM_MAGIC) return decoder_feed_transform(who, dec, (const uint8_t *)bytes, len, max_bits);
        if (bytes == nullptr || len < 4 || codec_read<uint32_t>((const uint8_t *)bytes) != INTER_MAGIC) return decoder_feed_plain(who, dec, bytes, len, false, max_bits);
        // an inter-frame packet: the container test, with the reference held, before anything is launched or allocated
        std::lock_guard<std::mutex> guard(dec->inter_lock);
        InterReference held;
        if (dec->reference) held = dec->reference->meta;
        InterLayout il;
        if (const char *problem = inter_validate((const uint8_t *)bytes, len, &held, il)) { note_error(who, problem); return -1; }
        if (il.total_bytes > 0x7fffffffull) { note_error(who, "the packet is too large"); return -1; }
        if (il.kind == INTER_KEY) return decoder_feed_plain(who, dec, (const uint8_t *)bytes + INTER_PREFIX_BYTES, len - INTER_PREFIX_BYTES, true, max_bits);
        return decoder_feed_delta(who, dec, (const uint8_t *)bytes, il, max_bits);
    });
}

extern "C" int cwipc_hip_decoder_set_max_octree_bits(cwipc_hip_decoder *dec, int bits) {
    const char *who = "cwipc_hip_decoder_set_max_octree_bits";
    if (dec == nullptr) { note_error(who, "NULL argument"); return -1; }
    if (bits < 0 || bits > CODEC_MAX_BITS) { note_error(who, "bits must be 0 (off) or in 1..16"); return -1; }
    dec->max_bits.store(bits);
    return 0;
}

extern "C" bool cwipc_hip_decoder_available(cwipc_hip_decoder *dec, bool wait) {
    if (dec == nullptr) return false;
    std::lock_guard<std::mutex> l(dec->lock);
    if (dec->queue.empty()) return false;
    const auto &planes = dec->queue.front().planes;
    if (!planes || !planes->ready) return true;
    if (wait) { planes->wait_host(); return true; }
    const hipError_t e = hipEventQuery(planes->ready);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
}

extern "C" cwipc_pointcloud *cwipc_hip_decoder_get(cwipc_hip_decoder *dec) {
    if (dec == nullptr) return nullptr;
    std::lock_guard<std::mutex> l(dec->lock);
    if (dec->queue.empty()) return nullptr;
    cwipc_hip_decoder::Job job = dec->queue.front();
    dec->queue.pop_front();
    release_upload(job);
    return job.cloud;
}

extern "C" bool cwipc_hip_decoder_eof(cwipc_hip_decoder *dec) {
    if (dec == nullptr) return true;
    std::lock_guard<std::mutex> l(dec->lock);
    return dec->closed && dec->queue.empty();
}

extern "C" void cwipc_hip_decoder_close(cwipc_hip_decoder *dec) {
    if (dec == nullptr) return;
    std::lock_guard<std::mutex> l(dec->lock);
    dec->closed = true;
}

extern "C" void cwipc_hip_decoder_free(cwipc_hip_decoder *dec) {
    if (dec == nullptr) return;
    for (auto &job : dec->queue) {
        release_upload(job);
        delete job.cloud;   // a result nobody took
    }
    delete dec;
}
