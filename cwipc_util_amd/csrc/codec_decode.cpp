// codec_decode.cpp -- the octree codec's decoder: cwipc_hip_new_decoder and its feed paths.  The interface is the one the reference's
// callers use (python/cwipc/net/source_decoder.py); the rule (RULE C: hip_ext.h, codec_terms.hpp) and the packets are this library's
// own and NOT interoperable with cwipc_codec.  Encoder: codec_encode.cpp; staging: codec_stage.hpp.
//
// Decode: validate on the host (nothing launched or allocated for a packet that is refused) -> upload -> the kernels, in flight
// when feed returns: the cloud carries a `ready` event.
//
// The entropy-coded form (RULE E: hip_ext.h, entropy_terms.hpp; kernels_entropy.hip): the container test on the host -> upload -> the
// streams decoded into the body buffer -> the check -> ONE wait in feed (a packet whose blocks or occupancy bytes fail is refused
// there) -> the decode above.
//
// Inter-frame coding (RULE P: hip_ext.h, inter_terms.hpp; kernels_inter.hip): the container test on the host -> upload -> the streams
// decoded, the added keys expanded, the checks -> ONE wait -> merge, rebuild, points.  The decoder keeps the frame's leaves on the
// device with the event of the work that made them.
//
// Transform colour coding (RULE T: hip_ext.h, transform_terms.hpp; kernels_transform.hip): the container test on the host -> upload ->
// the streams decoded, tokens and escapes joined and counted -> ONE wait -> the inverse transform into the body's colour plane -> the
// decode above.
//
// Level-of-detail decoding (RULE L: hip_ext.h, lod_terms.hpp; kernels_lod.hip).  A decoder told to hand out at most t octree bits does
// everything above up to the packet's body (or, for "cwap", the frame's leaves, which stay the FULL frame as the reference) and then,
// for a packet of b > t bits, makes the cloud of L(P, t) instead of the full one: the leaf runs of the nodes of depth t, the keys of
// depth t alone, the runs' sums, the points.  From a body nothing more is waited for; from a frame's leaves the number of runs is one
// more wait.  cwipc_hip_codec_lod (codec_host.cpp) is the host twin: it makes the packet L(P, t).
#include "codec_shared.hpp"

using namespace cwipc_amd;

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

// The cloud of dst's planes (their kernels queued on the calling thread's stream) onto the decoder's queue; job: the upload's
// staging buffer where the kernels read the packet from one.
int queue_cloud(cwipc_hip_decoder *dec, const std::shared_ptr<DeviceSoA> &dst, uint64_t timestamp, double cell, cwipc_hip_decoder::Job job = {}) {
    auto *cloud = new cwipc_hip_pointcloud();
    cloud->adopt_device(dst, timestamp, (float)cell);
    job.cloud = cloud;
    job.planes = dst;
    std::lock_guard<std::mutex> lk(dec->lock);
    dec->queue.push_back(job);
    return 0;
}

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
    DeviceBlocks blocks;
    uint8_t *block = blocks.alloc(start_bytes + cut_bytes + counts_bytes);
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
        if (!ok) hip_failed(hipGetLastError(), "octree decode (level of detail)", __FILE__, __LINE__);
        else note_error(who, "the leaf runs lost count");
        return nullptr;
    }
    auto dst = soa_alloc(nruns);
    k::CodecLeafSum *sums = (k::CodecLeafSum *)blocks.alloc(round256((size_t)nruns * sizeof(k::CodecLeafSum)));
    if (!dst || !sums) { note_error(who, "out of device memory"); return nullptr; }
    // (only bits, colour_bits, nleaves, the cube's corner and the cell are read of it)
    k::CodecDecode d = stage_decode_terms(l, t, l.colour_bits, codec_cellsize(l.side, t));
    d.nleaves = nruns;
    const k::LodSource src{leaves.n, l.colour_bits, 0, nullptr, 0, leaves.colour, leaves.tiles};
    blocks.queued = true;
    ok = k::lod_points(src, start, nruns, cut, sums, d, *dst, c.stream) && hipGetLastError() == hipSuccess;
    blocks.release();
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
    d.st.colour_bits = l.colour_bits;
    d.st.nleaves = l.nleaves;
    if (!stage_streams(el.stream, el.nstreams, [&](const EntropyStream &s) { return stage_offset_rule_e(l, s); }, d.st)) { note_error(who, STAGE_TOO_MANY_STREAMS); return false; }
    stage_decode_streams(el.stream, el.nstreams, el.directory_offset, d);
    CodedUpload up(el.total_bytes, el.directory_offset, d.st);
    const size_t channel_bytes = round256(3u * (size_t)l.nleaves), flag_bytes = round256(4u * (size_t)(1 + el.nstreams));
    if (!up.alloc(channel_bytes + flag_bytes, d)) { note_error(who, "out of memory"); return false; }
    d.channels = up.dev + up.upload_bytes;
    d.flags = (uint32_t *)(up.dev + up.upload_bytes + channel_bytes);
    d.occupancy = body;
    d.colours = (uint32_t *)(body + (l.colour_offset - l.occupancy_offset));
    d.tiles = body + (l.tile_offset - l.occupancy_offset);
    d.colour_words = codec_pad4(l.colour_bytes) / 4;
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 1);
    bool ok = up.send(bytes, el.directory_offset, el.stream, d.st, d.flags, flag_bytes, c.stream);
    if (ok) {
        k::entropy_decode(d, report.device(), tag, c.stream);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;   // the one wait: the streams are in `body`, the check's word is here
    if (!ok || !report.landed(tag, 0)) {
        hip_failed(hipGetLastError(), "octree decode (entropy stage)", __FILE__, __LINE__);
        return false;
    }
    if (const char *problem = stage_refusal(report.value(0))) { note_error(who, problem); return false; }
    return true;
}

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
    // the staging buffer of a "cwao" body: the decoder's queue keeps it until the cloud is taken, a feed that fails gives it back
    struct Staging {
        cwipc_hip_decoder::Job job;
        bool kept = false;
        ~Staging() { if (!kept && job.host) host_free(job.host, job.pinned); }
    } staging;
    cwipc_hip_decoder::Job &job = staging.job;
    std::shared_ptr<DeviceSoA> dst;   // (the cut of a key packet's frame is made from the reference's leaves, below)
    if (!(cut && keep_reference)) {
        dst = soa_alloc(cut ? l.nodes[out_bits - 1] : l.nleaves);
        if (!dst) { note_error(who, "out of device memory"); return -1; }
    }
    if (l.nleaves) {
        const size_t body = (size_t)(l.total_bytes - l.occupancy_offset);
        k::CodecDecode d = stage_decode_terms(l, l.bits, l.colour_bits, cell);
        const size_t body_bytes = round256(body + 8), ping_bytes = round256((size_t)l.nleaves * 8), scratch_bytes = round256(k::codec_decode_scratch_words(d) * 4);
        DeviceBlocks blocks;
        uint8_t *block = blocks.alloc(body_bytes + 2 * ping_bytes + scratch_bytes);
        if (!coded) job.host = (uint8_t *)host_alloc(body, &job.pinned);
        if (!block || (!coded && !job.host)) { note_error(who, "out of memory"); return -1; }
        d.colours = (const uint32_t *)(block + (l.colour_offset - l.occupancy_offset));
        d.tiles = l.tile_mode == 1 ? block + (l.tile_offset - l.occupancy_offset) : nullptr;
        bool ok = true;
        if (coded) {
            // the body comes from the entropy stage; a packet it refuses ends here, before any kernel of the octree decoder
            if (!entropy_to_body(who, c, (const uint8_t *)bytes, el, block)) return -1;
        } else {
            memcpy(job.host, (const uint8_t *)bytes + l.occupancy_offset, body);
            ok = hipMemcpyAsync(block, job.host, body, hipMemcpyHostToDevice, c.stream) == hipSuccess;
        }
        blocks.queued = true;
        if (ok) {
            unsigned long long *ping = (unsigned long long *)(block + body_bytes), *pong = (unsigned long long *)(block + body_bytes + ping_bytes);
            uint32_t *scratch = (uint32_t *)(block + body_bytes + 2 * ping_bytes);
            if (!cut) k::codec_decode(block, d, ping, pong, scratch, *dst, c.stream);
            else if (keep_reference) (void)k::codec_expand(block, d, ping, pong, scratch, c.stream);   // the full keys, for the reference
            else ok = lod_from_body(who, c, block, l, d, out_bits, nullptr, *dst);
            ok = ok && hipGetLastError() == hipSuccess;
        }
        blocks.release();   // (the kernels below still read `block`: it returns to the pool in the thread's next wait)
        if (!ok) {
            (void)c.sync();
            hip_failed(hipGetLastError(), "octree decode", __FILE__, __LINE__);
            return -1;
        }
        if (keep_reference) {
            // the leaves as the kernels above left them: the keys where the last depth's expansion wrote them
            std::unique_ptr<InterRefDev> next = InterRefDev::make(l);
            const uint8_t *leaf_keys = block + body_bytes + (l.bits % 2 ? ping_bytes : 0);
            if (!next || hipMemcpyAsync(next->leaves.keys, leaf_keys, 8u * (size_t)l.nleaves, hipMemcpyDeviceToDevice, c.stream) != hipSuccess) {
                (void)c.sync();
                note_error(who, "the reference could not be kept");
                return -1;
            }
            k::inter_leaves_of_planes(d.colours, d.colour_words, d.tiles, d.tile_value, l.colour_bits, next->leaves, c.stream);
            if (!next->published(c.stream)) (void)c.sync();
            replace_reference(dec->reference, std::move(next));
            if (cut) {
                dst = lod_from_leaves(who, c, dec->reference->leaves, l, out_bits);
                if (!dst) return -1;
            }
        }
        dst->mark_pending(c.stream);
    } else if (keep_reference) {
        replace_reference(dec->reference, nullptr);
    }
    const int rv = queue_cloud(dec, dst, l.timestamp, cell, job);
    staging.kept = true;
    return rv;
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
        const size_t n = l.nleaves, body = (size_t)(l.total_bytes - l.occupancy_offset);
        k::CodecDecode cd = stage_decode_terms(l, l.bits, 8, cell);
        // the entropy stage's streams: every stream but the escapes, which the transform's kernels read where the upload put them
        k::EntropyDecode d{};
        uint32_t escape_offset[3] = {0, 0, 0};
        for (int i = 0; i < tl.nstreams; i++)
            if (tl.stream[i].kind == TRANSFORM_ESCAPE) escape_offset[tl.stream[i].which] = (uint32_t)(tl.stream[i].payload_offset - tl.directory_offset);
        EntropyStream streams[TRANSFORM_MAX_STREAMS];
        const int nstreams = stage_without_escapes(tl.stream, tl.nstreams, streams);
        d.st.colour_bits = 8;
        d.st.nleaves = l.nleaves;
        if (!stage_streams(streams, nstreams, [&](const EntropyStream &s) { return stage_offset_rule_t(l, s); }, d.st)) { note_error(who, STAGE_TOO_MANY_STREAMS); return -1; }
        stage_decode_streams(streams, nstreams, tl.directory_offset, d);
        k::TransformTree tree{};
        k::transform_tree_counts(tree, l.bits, l.nodes, l.nleaves, tl.q16);
        const StageTreePlanes planes = stage_tree_planes(tree, nullptr, k::transform_scan_words(tree), false);
        const size_t body_bytes = round256(body + 8), ping_bytes = round256(n * 8), scratch_bytes = round256(k::codec_decode_scratch_words(cd) * 4),
                     flag_bytes = round256(4u * (size_t)(1 + d.st.nstreams));
        CodedUpload up(tl.total_bytes, tl.directory_offset, d.st);
        DeviceBlocks blocks;
        uint8_t *block = blocks.alloc(body_bytes + 2 * ping_bytes + scratch_bytes);
        uint8_t *tblock = blocks.alloc(planes.bytes);
        if (!up.alloc(flag_bytes, d) || !block || !tblock) { note_error(who, "out of memory"); return -1; }
        uint8_t *colours = block + (l.colour_offset - l.occupancy_offset);
        d.planes = tblock + planes.tokens;
        d.flags = (uint32_t *)(up.dev + up.upload_bytes);
        d.occupancy = block;
        d.tiles = block + (l.tile_offset - l.occupancy_offset);
        tree.occupancy = block;
        stage_tree_planes(tree, tblock, k::transform_scan_words(tree), false);
        PinnedReport report = c.report();
        const uint32_t tag = report.arm(0, 4);   // word 0: the entropy stage's status; words 1 .. 3: the tokens equal to 255 of Y, Co, Cg
        bool ok = up.send(bytes, tl.directory_offset, streams, d.st, d.flags, flag_bytes, c.stream);
        if (ok) {
            k::entropy_decode(d, report.device(), tag, c.stream);
            k::transform_prepare(tree, c.stream);
            k::transform_untoken(tree, d.planes, up.dev, escape_offset, tl.nescapes, report.device() + 1, tag, c.stream);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = c.sync() && ok;   // the one wait
        up.sent();
        if (!ok || !report.landed(tag, 0, 4)) {
            hip_failed(hipGetLastError(), "octree decode (transform stage)", __FILE__, __LINE__);
            return -1;
        }
        const char *problem = stage_refusal(report.value(0));
        for (int ch = 0; ch < 3 && !problem; ch++)
            if (report.value(1 + ch) != tl.nescapes[ch]) problem = "tokens equal to 255 differ from the escape count";
        if (problem) { note_error(who, problem); return -1; }
        cd.colours = (const uint32_t *)colours;
        cd.tiles = l.tile_mode == 1 ? d.tiles : nullptr;
        blocks.queued = up.queued = true;
        k::transform_inverse(tree, tl.dc, colours, c.stream);
        if (cut) ok = lod_from_body(who, c, block, l, cd, out_bits, tree.first, *dst);
        else k::codec_decode(block, cd, (unsigned long long *)(block + body_bytes), (unsigned long long *)(block + body_bytes + ping_bytes),
                             (uint32_t *)(block + body_bytes + 2 * ping_bytes), *dst, c.stream);
        ok = ok && hipGetLastError() == hipSuccess;
        blocks.release();
        up.release();
        if (!ok) {
            (void)c.sync();
            hip_failed(hipGetLastError(), "octree decode", __FILE__, __LINE__);
            return -1;
        }
        dst->mark_pending(c.stream);
    }
    return queue_cloud(dec, dst, l.timestamp, cell);
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
    d.st.colour_bits = l.colour_bits;
    d.st.nleaves = l.nleaves;
    const auto rule_p = [&](const EntropyStream &s) { return stage_offset_rule_p(il.nodes_added, res_offset, n, s); };
    if (!stage_streams(il.stream, il.nstreams, rule_p, d.st)) { note_error(who, STAGE_TOO_MANY_STREAMS); return -1; }
    stage_decode_streams(il.stream, il.nstreams, il.directory_offset, d);
    k::CodecDecode added_tree{};   // the tree of the added leaves, for codec_expand
    added_tree.bits = l.bits;
    added_tree.nleaves = il.nadded;
    for (int i = 0; i < l.bits; i++) added_tree.nodes[i] = il.nodes_added[i];
    const uint64_t occupancy_bytes = nadded ? inter_depth_offset(il.nodes_added, l.bits - 1) + (l.bits > 1 ? il.nodes_added[l.bits - 2] : 1u) : 0u;
    CodedUpload up(il.total_bytes, il.directory_offset, d.st);
    const size_t occupancy_block = round256((size_t)occupancy_bytes + 8), ping_bytes = round256(8 * nadded + 8),
                 scratch_bytes = round256(k::codec_decode_scratch_words(added_tree) * 4), nrb = k::codec_blocks(nr),
                 rank_bytes = round256((nr + 1) * 4), counts_bytes = round256((nrb + 1) * 4), flag_bytes = 256;
    const size_t planes_at = up.upload_bytes, occupancy_at = planes_at + planes_bytes, ping_at = occupancy_at + occupancy_block, scratch_at = ping_at + 2 * ping_bytes,
                 rank_at = scratch_at + scratch_bytes, counts_at = rank_at + rank_bytes, flags_at = counts_at + counts_bytes;
    if (!up.alloc(flags_at + flag_bytes - up.upload_bytes, d)) { note_error(who, "out of memory"); return -1; }
    uint8_t *dev = up.dev;
    d.planes = dev + planes_at;
    d.occupancy = dev + occupancy_at;
    d.flags = (uint32_t *)(dev + flags_at);   // words 0 .. S: the entropy stage's; word 32: the checks'
    const uint8_t *keep = d.planes, *res = d.planes + res_offset;
    unsigned long long *ping = (unsigned long long *)(dev + ping_at), *pong = (unsigned long long *)(dev + ping_at + ping_bytes);
    uint32_t *rank = (uint32_t *)(dev + rank_at);
    R.wait_on(c.stream);
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 3);   // word 0: the entropy stage's status; word 1: the checks'; word 2: the kept leaves
    bool ok = up.send(bytes, il.directory_offset, il.stream, d.st, d.flags, flag_bytes, c.stream);
    const unsigned long long *added = ping;
    if (ok) {
        k::entropy_decode(d, report.device(), tag, c.stream);
        if (nadded) added = k::codec_expand(d.occupancy, added_tree, ping, pong, (uint32_t *)(dev + scratch_at), c.stream);
        k::inter_check(R.leaves, keep, added, il.nadded, l.nleaves, rank, (uint32_t *)(dev + counts_at), d.flags + 32, report.device() + 1, tag, c.stream);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;   // the one wait: the streams are in their planes, the two status words are here
    up.sent();
    if (!ok || !report.landed(tag, 0) || !report.landed(tag, 1)) {
        hip_failed(hipGetLastError(), "octree decode (delta)", __FILE__, __LINE__);
        return -1;
    }
    if (const char *problem = stage_refusal(report.value(0) | report.value(1))) { note_error(who, problem); return -1; }
    const double cell = codec_cellsize(l.side, l.bits);
    auto dst = soa_alloc(l.nleaves);
    std::unique_ptr<InterRefDev> next = InterRefDev::make(l);
    if (!dst || !next) { note_error(who, "out of device memory"); return -1; }
    // (a delta's header carries no nodes[] and no offsets: the terms are the bit counts, the tile value, the leaf count and the cube)
    const k::CodecDecode points = stage_decode_terms(l, l.bits, l.colour_bits, cell);
    up.queued = true;
    k::inter_apply(R.leaves, keep, rank, added, il.nadded, res, points, l.tile_mode, next->leaves, *dst, c.stream);
    ok = hipGetLastError() == hipSuccess && next->published(c.stream);
    up.release();
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
    return queue_cloud(dec, dst, l.timestamp, codec_cellsize(l.side, out_bits));
}

}  // namespace

extern "C" cwipc_hip_decoder *cwipc_hip_new_decoder(char **errorMessage) {
    ErrorbufScope scope(errorMessage);
    cwipc_hip_decoder *d = new (std::nothrow) cwipc_hip_decoder();
    if (!d) note_error("cwipc_hip_new_decoder", "out of memory");
    return d;
}

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
    return event_done(planes->ready, false);
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

extern "C" bool cwipc_hip_decoder_eof(cwipc_hip_decoder *dec) { return queue_eof(dec); }

extern "C" void cwipc_hip_decoder_close(cwipc_hip_decoder *dec) { queue_close(dec); }

extern "C" void cwipc_hip_decoder_free(cwipc_hip_decoder *dec) {
    if (dec == nullptr) return;
    for (auto &job : dec->queue) {
        release_upload(job);
        delete job.cloud;   // a result nobody took
    }
    delete dec;
}
