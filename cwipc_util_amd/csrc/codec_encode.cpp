// codec_encode.cpp -- the octree codec's encoder: cwipc_hip_new_encoder, cwipc_hip_new_encodergroup and their host orchestration.  The
// interface is the one the reference's callers use (python/cwipc/net/sink_encoder.py); the rule (RULE C: hip_ext.h, codec_terms.hpp) and
// the packets are this library's own and NOT interoperable with cwipc_codec.  Decoder: codec_decode.cpp; staging: codec_stage.hpp.
//
// Encode: filter -> cube, keys, sort, per-depth counts and their scan -> ONE wait (nodes[] and the cube size the packet) -> the
// body's kernels and its copy into page-locked memory, in flight when feed returns.  The header is written by the host; the tile
// mode, known only when the leaves are, is filled in when the result is taken.
//
// The entropy-coded form (RULE E: hip_ext.h, entropy_terms.hpp; kernels_entropy.hip): the entropy stage runs on the body the device
// holds after codec_leaf; its size is the device's to find, so feed queues the stage and a copy of four report words and returns;
// whoever polls or takes the result first waits for those words and issues the copy of exactly the packet's bytes (EncJob: stage
// 0 -> 1), and takes it when that copy is done.
//
// Inter-frame coding (RULE P: hip_ext.h, inter_terms.hpp; kernels_inter.hip): one wave behind the cube kernel decides between key
// and delta and leaves the cube to quantise in; the choice rides to the host with the cube in the sort's one wait.  A key frame is
// the packet above behind a prefix; its leaves are taken out of the body as the next reference.  A delta frame matches the frame's
// leaves against the reference on the device and WAITS A SECOND TIME for the number of added leaves and their node counts, which
// size the entropy stage's streams; from there on it is the entropy-coded form's path (report, then the copy of exactly the
// packet's bytes).  The encoder keeps the frame's leaves on the device with the event of the work that made them.
//
// Transform colour coding (RULE T: hip_ext.h, transform_terms.hpp; kernels_transform.hip): behind codec_emit at shift 0 the leaves'
// colours become coefficients, their tokens go through the entropy stage with occupancy and tiles, and one more kernel puts the
// packet together around the escape streams, whose sizes only the device knows; the size arrives as the entropy-coded form's does.
#include "codec_shared.hpp"

using namespace cwipc_amd;

namespace {

// One encoded packet, possibly still being written by the device.
struct EncJob {
    uint8_t *host = nullptr;
    bool pinned = false;
    CodecLayout layout;              // tile_mode 1 until finalize() has looked at the leaves
    size_t tile_words_at = 0;        // where the two tile words land in `host` (0: an empty cloud, nothing in flight)
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
    // the entropy stage's four report words (the bytes that count, S, the two tile words) land at `offset` in `host`
    void report_at(size_t offset) { report_offset = offset, tile_words_at = offset + 8; }
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
    void finalize() {
        if (final) return;
        if (done) {
            if (stage == 0) (void)hipEventSynchronize(done);
            if (entropy && stage == 0) start_copy();
            if (copied) { (void)hipEventSynchronize(copied); event_put(copied); copied = nullptr; }
            event_put(done);
            done = nullptr;
        }
        src.reset();
        if (out_dev) { pool_free(out_dev); out_dev = nullptr; }
        uint32_t words[2] = {0, 0};   // (an empty cloud: tile mode 0, tile value 0)
        if (tile_words_at) memcpy(words, host + tile_words_at, 8);
        stage_tile_words(words[0], words[1], layout.tile_mode, layout.tile_value);
        host[tile_at] = (uint8_t)layout.tile_mode;
        host[tile_at + 1] = (uint8_t)layout.tile_value;
        if (entropy) {
            if (!report_offset) out_bytes = empty_bytes;   // an empty cloud: S = 0, written with the header
            layout.total_bytes = failed ? 0u : (uint64_t)(head_bytes() + out_bytes);
            if (failed) note_error("octree encode", "the entropy stage failed");
        } else {
            codec_layout_sizes(layout);
        }
        final = true;
    }
};

// A cloud sorted for `bits`, with what the one read-back brought.  Its block goes back in the calling thread's next wait: the
// packets' kernels, queued by then, read it.
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
    ~Sorted() { tctx().free_later(block); }
};

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

// A packet's body on the device: occupancy, colours, the tile plane and the two tile words (`bytes`), and behind them the leaf sums.
// What goes behind it (the copy out, the entropy stage, the transform stage around that) reads it where codec_emit left it.
struct Body {
    size_t bytes, sums_offset, block_bytes;
    uint8_t *block = nullptr;
    k::CodecEmit e{};
    explicit Body(const CodecLayout &l)
        : bytes((size_t)(l.tile_offset - l.occupancy_offset) + (size_t)codec_pad4(l.nleaves) + 8), sums_offset((bytes + 7) & ~(size_t)7),
          block_bytes(sums_offset + (size_t)l.nleaves * sizeof(k::CodecLeafSum)) {}
    // the block, and where codec_emit writes in it (zeroed): the body, then the leaf sums at sums_offset
    bool alloc(const CodecLayout &l, DeviceBlocks &blocks) {
        block = blocks.alloc(block_bytes);
        if (!block) return false;
        e.bits = l.bits;
        e.nleaves = l.nleaves;
        e.depth_offset[0] = 0;
        for (int L = 1; L < l.bits; L++) e.depth_offset[L] = L == 1 ? 1u : e.depth_offset[L - 1] + l.nodes[L - 2];
        e.occupancy_bytes = l.occupancy_bytes;
        e.colour_words = codec_pad4(l.colour_bytes) / 4;
        e.occupancy = (uint32_t *)block;
        e.colours = (uint32_t *)(block + (l.colour_offset - l.occupancy_offset));
        e.tiles = block + (l.tile_offset - l.occupancy_offset);
        e.tile_stats = (uint32_t *)(block + bytes - 8);
        e.sums = (k::CodecLeafSum *)(block + sums_offset);
        return true;
    }
    // onto the calling thread's stream: the zeroed block, codec_emit and, with `leaves` (RULE P), the frame's leaves out of the body
    bool queue(ThreadCtx &c, const Sorted &s, int shift, int colour_bits, const k::InterLeavesDev *leaves) const {
        if (hipMemsetAsync(block, 0, block_bytes, c.stream) != hipSuccess) return false;
        k::codec_emit(s.keys + s.n, s.index + s.n, *s.src, s.cube_dev, s.bits, s.counts, e, shift, c.stream);
        if (leaves) k::inter_leaves_of_body(s.keys + s.n, s.n, s.cube_dev, s.counts, e, colour_bits, *leaves, c.stream);
        return true;
    }
};

// Behind the body, the plain form: its bytes into the packet behind the header.
bool copy_out_body(ThreadCtx &c, EncJob &job, const Body &body) {
    job.tile_words_at = (size_t)job.layout.occupancy_offset + body.bytes - 8;
    return hipMemcpyAsync(job.host + job.layout.occupancy_offset, body.block, body.bytes, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
}

// Behind the body (or RULE P's planes), the entropy stage: en.st, the planes it reads, `out` and its capacity are the caller's.  Here
// the work block is carved and what the stage wants zeroed is; k::entropy_encode follows once the kernels that make its planes are queued.
bool entropy_stage_zeroed(ThreadCtx &c, k::EntropyEncode &en, uint8_t *work) {
    stage_encode_work(en, work);
    return hipMemsetAsync(en.hist, 0, (size_t)en.st.nstreams * 1024, c.stream) == hipSuccess && hipMemsetAsync(en.out, 0, en.out_capacity, c.stream) == hipSuccess;
}

// only the packet's own bytes cross the bus: here the four report words, the rest when the result is polled or taken
bool copy_report(ThreadCtx &c, EncJob &job, const uint32_t *report) {
    return hipMemcpyAsync(job.host + job.report_offset, report, 16, hipMemcpyDeviceToHost, c.stream) == hipSuccess && hipGetLastError() == hipSuccess;
}

// Behind the body, RULE T around the entropy stage: the coefficients of the leaves' colours, their tokens as the stage's byte
// planes, the stage into en.out (a block of its own), and the packet put together from that in the job's `out`.  tblock: the tree's planes.
bool transform_stage(ThreadCtx &c, EncJob &job, const Body &body, k::TransformTree &tree, const StageTreePlanes &planes, uint8_t *tblock, uint32_t q16,
                     k::EntropyEncode &en, uint8_t *work) {
    const CodecLayout &l = job.layout;
    tree.occupancy = en.occupancy;
    uint8_t *tokens = tblock + planes.tokens;
    uint16_t *escapes = (uint16_t *)(tblock + planes.escapes);
    if (!entropy_stage_zeroed(c, en, work) || hipMemsetAsync(escapes, 0, 6 * (size_t)planes.escape_stride, c.stream) != hipSuccess) return false;
    k::transform_prepare(tree, c.stream);
    k::transform_forward(tree, (const uint8_t *)body.e.colours, c.stream);
    k::transform_tokens(tree, tokens, escapes, planes.escape_stride, c.stream);
    en.planes = tokens;
    k::entropy_encode(en, c.stream);
    k::TransformAssemble a{};
    a.bits = l.bits;
    a.entropy_streams = en.st.nstreams;
    a.plan = en.plan;
    a.in_report = en.report;
    a.in = en.out;
    a.escapes = escapes;
    a.escape_stride = planes.escape_stride;
    for (int ch = 0; ch < 3; ch++) {
        a.escape_total[ch] = k::transform_escape_total(tree, ch);
        a.dc[ch] = tree.value + (size_t)ch * ((size_t)tree.inner + l.nleaves);
    }
    a.q16 = q16;
    a.out = (uint8_t *)job.out_dev;
    a.out_capacity = job.out_capacity;
    a.report = (uint32_t *)(tblock + planes.report);
    k::transform_assemble(a, c.stream);
    return copy_report(c, job, a.report);
}

// the job's kernels are queued: its event, and the blocks back to the pool in the thread's next wait
std::unique_ptr<EncJob> emitted(const char *what, ThreadCtx &c, std::unique_ptr<EncJob> job, const Sorted &s, DeviceBlocks &blocks, bool ok, int line) {
    job->done = event_get();
    ok = ok && job->done && hipEventRecord(job->done, c.stream) == hipSuccess;
    blocks.release();
    if (!ok) {
        (void)c.sync();
        hip_failed(hipGetLastError(), what, __FILE__, line);
        return nullptr;
    }
    job->src = s.src;
    return job;
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
    Body body(l);
    const bool transform = transform_q16 != 0u;
    // the entropy-coded form: its streams (with a tile plane, which the plan kernel drops when the tiles turn out uniform) and the
    // most bytes it can take from the word S on
    k::EntropyEncode en{};
    size_t entropy_capacity = 0;   // of the entropy stage's own output
    if (entropy) {
        EntropyStream streams[TRANSFORM_MAX_STREAMS];
        // RULE T: occupancy, the three token planes and the tile plane go through the stage; the escape streams join them afterwards
        const uint32_t none[3] = {0, 0, 0};
        const int nstreams = transform ? stage_without_escapes(streams, transform_streams(l, none, streams), streams) : entropy_streams(l, streams);
        en.st.colour_bits = l.colour_bits;
        en.st.nleaves = l.nleaves;
        entropy_capacity = stage_streams(streams, nstreams, [&](const EntropyStream &es) { return transform ? stage_offset_rule_t(l, es) : stage_offset_rule_e(l, es); }, en.st);
        if (!entropy_capacity) { note_error(who, STAGE_TOO_MANY_STREAMS); return nullptr; }
        if (entropy_capacity > 0x7fffffffull) { note_error(who, "the cloud is too large for the entropy-coded form"); return nullptr; }
        job->entropy = true;
        job->out_capacity = entropy_capacity;
        if (transform) {
            // what the packet can take from the fixed bytes on: three more directory entries and every coefficient an escape
            const size_t most = TRANSFORM_FIXED_BYTES + entropy_capacity + (l.nleaves ? 24u + 3u * (size_t)codec_pad4(2u * ((size_t)l.nleaves - 1u)) : 0u);
            if (most > 0x7fffffffull || (uint64_t)l.occupancy_bytes + l.nleaves > 0x7fffffffull) { note_error(who, "the cloud is too large for the transform-coded form"); return nullptr; }
            job->out_capacity = most;
            job->empty_bytes = TRANSFORM_FIXED_BYTES + 4u;
        }
    }
    job->host = (uint8_t *)host_alloc(prefix + (size_t)l.occupancy_offset + (entropy ? job->out_capacity + 16 : body.bytes), &job->pinned);
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
    // every block before anything is queued
    DeviceBlocks blocks;
    k::TransformTree tree{};
    StageTreePlanes planes{};
    uint8_t *work = nullptr, *tblock = nullptr;
    if (!body.alloc(l, blocks)) { note_error(who, "out of device memory"); return nullptr; }
    bool have = true;
    if (transform) {
        k::transform_tree_counts(tree, l.bits, l.nodes, l.nleaves, transform_q16);
        planes = stage_tree_planes(tree, nullptr, k::transform_scan_words(tree), true);
        tblock = blocks.alloc(planes.bytes);
        if (tblock) stage_tree_planes(tree, tblock, k::transform_scan_words(tree), true);
        en.out = blocks.alloc(round256(entropy_capacity));   // the stage's output, which transform_assemble reads
        have = tblock && en.out;
    }
    if (entropy) {
        work = blocks.alloc(stage_encode_work(en, nullptr));
        job->out_dev = pool_alloc(round256(job->out_capacity));
        if (!transform) en.out = (uint8_t *)job->out_dev;
        have = have && work && job->out_dev;
    }
    if (!have) { note_error(who, "out of device memory"); return nullptr; }
    blocks.queued = true;
    bool ok = body.queue(c, s, shift, l.colour_bits, key_leaves);
    if (ok && !entropy) {
        ok = copy_out_body(c, *job, body) && hipGetLastError() == hipSuccess;
    } else if (ok) {
        ok = hipGetLastError() == hipSuccess;
        en.occupancy = (const uint8_t *)body.e.occupancy;
        en.tiles = body.e.tiles;
        en.colours = body.e.colours;
        en.tile_stats = body.e.tile_stats;
        en.colour_words = body.e.colour_words;
        en.out_capacity = entropy_capacity;
        job->report_at((size_t)l.occupancy_offset + (size_t)codec_pad4(job->out_capacity));
        if (ok && transform) ok = transform_stage(c, *job, body, tree, planes, tblock, transform_q16, en, work);
        else if (ok && (ok = entropy_stage_zeroed(c, en, work))) {
            k::entropy_encode(en, c.stream);
            ok = copy_report(c, *job, en.report);
        }
    }
    return emitted("octree encode", c, std::move(job), s, blocks, ok, __LINE__);
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
    Body body(l);
    // the planes the entropy stage reads: keep, then the four residual planes; behind them what the match and the count of A need
    const size_t keep_bytes = (nr + 7) / 8, res_offset = round256(keep_bytes), added_offset = res_offset + round256(4 * n),
                 counts_offset = added_offset + round256(9 * n), counts_added_offset = counts_offset + round256((nb + 1) * 4),
                 cube_offset = counts_added_offset + round256((size_t)bits * (nb + 1) * 4), match_bytes = cube_offset + 256;
    if (match_bytes > 0x7fffffffull) { note_error(who, "the cloud is too large for a delta packet"); return nullptr; }
    // (given back by hand until the wait below is over: a block handed to free_later would return to the pool in it)
    DeviceBlocks blocks;
    uint8_t *match = blocks.alloc(match_bytes);
    if (!match || !body.alloc(l, blocks)) { note_error(who, "out of device memory"); return nullptr; }
    unsigned long long *added = (unsigned long long *)(match + added_offset);
    uint32_t *counts_added = (uint32_t *)(match + counts_added_offset);
    k::CodecCube *cube_added = (k::CodecCube *)(match + cube_offset);
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 17);   // words 0 .. bits - 1: nodesA[]; word 16: nadded
    bool ok = body.queue(c, s, shift, l.colour_bits, &P);
    if (ok) {
        k::inter_match(R.leaves, P, l.colour_bits, match, match + res_offset, added, (uint32_t *)(match + counts_offset), cube_added, report.device() + 16, tag,
                       c.stream);
        k::codec_count_scan(added, n, cube_added, bits, counts_added, report.device(), tag, c.stream);
        ok = hipMemcpyAsync(c.host_words + 40, body.e.tile_stats, 8, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
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
    stage_tile_words(stats[0], stats[1], l.tile_mode, l.tile_value);
    if (nadded > n || (nadded ? nodes_added[bits - 1] != nadded : nodes_added[bits - 1] != 0u)) { note_error(who, "the match lost count of the added leaves"); return nullptr; }
    // the streams, now that every count is known, and the most bytes the packet can take from the word S on
    EntropyStream streams[INTER_MAX_STREAMS];
    k::EntropyEncode en{};
    en.st.colour_bits = l.colour_bits;
    en.st.nleaves = l.nleaves;
    const int nstreams = inter_streams((uint32_t)nr, l.nleaves, bits, l.colour_bits, l.tile_mode, nadded, nodes_added, streams);
    const size_t out_capacity = stage_streams(streams, nstreams, [&](const EntropyStream &es) { return stage_offset_rule_p(nodes_added, res_offset, n, es); }, en.st);
    if (!out_capacity) { note_error(who, STAGE_TOO_MANY_STREAMS); return nullptr; }
    if (out_capacity > 0x7fffffffull) { note_error(who, "the cloud is too large for a delta packet"); return nullptr; }
    const size_t head = INTER_PREFIX_BYTES + INTER_HEADER_BYTES + 4u + 4u * (size_t)bits;
    job->entropy = true;
    job->out_capacity = out_capacity;
    job->head = head;
    job->tile_at = INTER_PREFIX_BYTES + 22 - 8;
    job->report_at(head + (size_t)codec_pad4(out_capacity));
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
    uint8_t *occupancy = blocks.alloc(occupancy_block);
    uint8_t *work = blocks.alloc(stage_encode_work(en, nullptr));
    job->out_dev = pool_alloc(round256(out_capacity));
    if (!occupancy || !work || !job->out_dev) { note_error(who, "out of device memory"); return nullptr; }
    en.planes = match;
    en.occupancy = occupancy;
    en.tile_stats = body.e.tile_stats;
    en.out = (uint8_t *)job->out_dev;
    en.out_capacity = out_capacity;
    blocks.queued = true;
    ok = hipMemsetAsync(occupancy, 0, occupancy_block, c.stream) == hipSuccess && entropy_stage_zeroed(c, en, work);
    if (ok) {
        k::inter_occupancy(added, nadded, n, bits, counts_added, depth_offset, occupancy_bytes, (uint32_t *)occupancy, c.stream);
        k::entropy_encode(en, c.stream);
        ok = copy_report(c, *job, en.report);
    }
    return emitted("octree encode (delta)", c, std::move(job), s, blocks, ok, __LINE__);
}

// The clouds filtered_input makes on the way: they go when the feed that asked for them is over (the planes stay with the packet's job).
struct MadeClouds {
    std::vector<cwipc_pointcloud *> list;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    ~MadeClouds() { for (cwipc_pointcloud *p : list) delete p; }
};

// The cloud an encoder of (tilenumber, voxelsize) works on, on the device.
std::shared_ptr<DeviceSoA> filtered_input(const char *who, cwipc_pointcloud *pc, int tilenumber, float voxelsize, MadeClouds &made) {
    cwipc_pointcloud *cur = pc;
    if (tilenumber != 0) {
        cur = cwipc_tilefilter(cur, tilenumber);
        if (!cur) { note_error(who, "cwipc_tilefilter failed"); return nullptr; }
        made.list.push_back(cur);
    }
    if (voxelsize > 0) {
        cur = cwipc_downsample(cur, voxelsize);
        if (!cur) { note_error(who, "cwipc_downsample failed"); return nullptr; }
        made.list.push_back(cur);
    }
    cwipc_hip_pointcloud *ours = as_ours(cur);
    if (!ours) {
        made.keep = import_foreign(cur);
        ours = made.keep.get();
    }
    if (!ours || !ours->has_data()) { note_error(who, "cannot read the point data of the argument"); return nullptr; }
    if (!device_available(who)) return nullptr;
    auto dev = ours->device_points();
    if (!dev) note_error(who, "the cloud cannot be brought to the device");
    return dev;
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

namespace {

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
        int rv = -1;
        auto src = filtered_input(who, pc, enc->params.tilenumber, enc->params.voxelsize, made);
        if (src && enc->inter) {
            rv = encoder_feed_inter(who, enc, src, pc->timestamp());
        } else if (src) {
            Sorted s;
            if (sort_cloud(who, src, enc->params.octree_bits, s)) rv = encoder_feed_sorted(who, enc, s, pc->timestamp());
        }
        return rv;
    });
}

// the packet form is chosen before the first feed; not_with_inter: why the form is not to be had in inter mode, or nullptr
static int choose_form(const char *who, cwipc_hip_encoder *enc, bool cwipc_hip_encoder::*form, int on, const char *not_with_inter) {
    if (enc == nullptr) { note_error(who, "NULL argument"); return -1; }
    std::lock_guard<std::mutex> l(enc->lock);
    if (enc->fed) { note_error(who, "the encoder has been fed: the packet form is chosen before the first feed"); return -1; }
    if (on != 0 && enc->inter && not_with_inter) { note_error(who, not_with_inter); return -1; }
    enc->*form = on != 0;
    return 0;
}

extern "C" int cwipc_hip_encoder_set_entropy(cwipc_hip_encoder *enc, int on) {
    return choose_form("cwipc_hip_encoder_set_entropy", enc, &cwipc_hip_encoder::entropy, on, nullptr);
}

extern "C" int cwipc_hip_encoder_set_colour_transform(cwipc_hip_encoder *enc, int on) {
    return choose_form("cwipc_hip_encoder_set_colour_transform", enc, &cwipc_hip_encoder::transform, on,
                       "inter mode: a delta's colour differences are exact residuals to the reference; transform colour under RULE P is out of scope");
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

extern "C" bool cwipc_hip_encoder_eof(cwipc_hip_encoder *enc) { return queue_eof(enc); }

extern "C" void cwipc_hip_encoder_close(cwipc_hip_encoder *enc) { queue_close(enc); }

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
    const auto refused = [&](const char *why) -> cwipc_hip_encoder * {
        ErrorbufScope scope(errorMessage);
        note_error("cwipc_hip_encodergroup_addencoder", why);
        return nullptr;
    };
    if (group == nullptr) return refused("NULL argument");
    if (params != nullptr && inter_params_on(params->do_inter_frame, params->gop_size, params->exp_factor))
        return refused("do_inter_frame: inter-frame coding is not available inside an encoder group (out of scope)");
    cwipc_hip_encoder *enc = cwipc_hip_new_encoder(params, errorMessage);
    if (!enc) return nullptr;
    enc->in_group = true;
    std::lock_guard<std::mutex> l(group->lock);
    try {
        group->encoders.push_back(enc);
    } catch (...) {
        delete enc;
        return refused("out of memory");
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
            int bits = 0;
            for (cwipc_hip_encoder *enc : cls) bits = enc->params.octree_bits > bits ? enc->params.octree_bits : bits;
            auto src = filtered_input(who, pc, cls[0]->params.tilenumber, cls[0]->params.voxelsize, made);
            Sorted s;
            if (src && sort_cloud(who, src, bits, s)) {
                for (cwipc_hip_encoder *enc : cls)
                    if (encoder_feed_sorted(who, enc, s, pc->timestamp()) != 0) rv = -1;
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
