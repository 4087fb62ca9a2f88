// codec_host.cpp -- the octree codec's entry points that never touch the GPU: what a packet's header and stream directory say
// (cwipc_hip_codec_packet_info, _entropy_info, _transform_info, _inter_info) and the conversions between the packet forms, which
// are the terms headers' host twins of the kernels (RULE E, T, P and L: hip_ext.h).  Encoder: codec_encode.cpp; decoder: codec_decode.cpp.
#include "codec_shared.hpp"

using namespace cwipc_amd;

namespace {

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

// the stream directory of a validated layout into an info struct's arrays (`kind`: the streams' kinds, which RULE P's struct names kind_of)
template <typename Layout, typename Info>
void fill_directory(const Layout &e, Info *info, int32_t *kind) {
    info->nstreams = e.nstreams;
    for (int i = 0; i < e.nstreams; i++) {
        kind[i] = (int32_t)e.stream[i].kind;
        info->which[i] = (int32_t)e.stream[i].which;
        info->mode[i] = (int32_t)e.stream[i].mode;
        info->symbols[i] = e.stream[i].symbols;
        info->payload_offset[i] = e.stream[i].payload_offset;
        info->payload_bytes[i] = e.stream[i].payload_bytes;
    }
    info->total_bytes = e.total_bytes;
}

// A packet's container test behind the C boundary: validate(layout) returns why not, or nullptr; then the header's fields of the
// packet it stands for, and what `more` adds of the layout.
template <typename Layout, typename Info, typename Validate, typename More>
int info_of(const char *who, Info *info, char **errorMessage, Validate &&validate, More &&more) {
    ErrorbufScope scope(errorMessage);
    Layout e;
    if (const char *problem = validate(e)) { note_error(who, problem); return -1; }
    if (info) {
        memset(info, 0, sizeof(*info));
        fill_info(e.cwao, &info->packet);
        more(e);
    }
    return 0;
}

// One host conversion behind the C boundary: convert(made) returns why not, or nullptr with the packet in `made`.  The caller-buffer
// convention: the size of the result; its bytes are written iff they fit.
template <typename Convert>
size_t converted(const char *who, void *out, size_t capacity, char **errorMessage, Convert &&convert) {
    ErrorbufScope scope(errorMessage);
    return guarded(who, (size_t)0, [&]() -> size_t {
        std::vector<uint8_t> made;
        if (const char *problem = convert(made)) { note_error(who, problem); return 0; }
        if (out != nullptr && made.size() <= capacity) memcpy(out, made.data(), made.size());
        return made.size();
    });
}

}  // namespace

extern "C" int cwipc_hip_codec_packet_info(const void *bytes, size_t len, cwipc_hip_codec_info *info, char **errorMessage) {
    const char *who = "cwipc_hip_codec_packet_info";
    ErrorbufScope scope(errorMessage);
    CodecLayout l;
    if (const char *problem = codec_validate((const uint8_t *)bytes, len, l)) { note_error(who, problem); return -1; }
    if (info) fill_info(l, info);
    return 0;
}

// ---- the entropy-coded form ----
extern "C" size_t cwipc_hip_codec_entropy_pack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage) {
    return converted("cwipc_hip_codec_entropy_pack", out, capacity, errorMessage, [&](auto &made) { return entropy_pack((const uint8_t *)bytes, len, made); });
}

extern "C" size_t cwipc_hip_codec_entropy_unpack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage) {
    return converted("cwipc_hip_codec_entropy_unpack", out, capacity, errorMessage, [&](auto &made) { return entropy_unpack((const uint8_t *)bytes, len, made); });
}

extern "C" int cwipc_hip_codec_entropy_info(const void *bytes, size_t len, cwipc_hip_codec_entropy_directory *info, char **errorMessage) {
    return info_of<EntropyLayout>("cwipc_hip_codec_entropy_info", info, errorMessage, [&](EntropyLayout &e) { return entropy_validate((const uint8_t *)bytes, len, e); },
                                  [&](const EntropyLayout &e) { fill_directory(e, info, info->kind); });
}

// ---- transform colour coding ----
extern "C" size_t cwipc_hip_codec_transform_pack(const void *bytes, size_t len, int jpeg_quality, void *out, size_t capacity, char **errorMessage) {
    return converted("cwipc_hip_codec_transform_pack", out, capacity, errorMessage,
                     [&](auto &made) { return transform_pack((const uint8_t *)bytes, len, jpeg_quality, made); });
}

extern "C" size_t cwipc_hip_codec_transform_unpack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage) {
    return converted("cwipc_hip_codec_transform_unpack", out, capacity, errorMessage, [&](auto &made) { return transform_unpack((const uint8_t *)bytes, len, made); });
}

extern "C" int cwipc_hip_codec_transform_info(const void *bytes, size_t len, cwipc_hip_codec_transform_directory *info, char **errorMessage) {
    return info_of<TransformLayout>("cwipc_hip_codec_transform_info", info, errorMessage, [&](TransformLayout &t) { return transform_validate((const uint8_t *)bytes, len, t); },
                                    [&](const TransformLayout &t) {
                                        info->q16 = t.q16;
                                        for (int ch = 0; ch < 3; ch++) {
                                            info->dc[ch] = t.dc[ch];
                                            info->nescapes[ch] = t.nescapes[ch];
                                        }
                                        fill_directory(t, info, info->kind);
                                    });
}

// ---- inter-frame packets ----
extern "C" size_t cwipc_hip_codec_inter_pack(const void *r, size_t rlen, const void *p, size_t plen, uint32_t gop_index, void *out, size_t capacity,
                                             char **errorMessage) {
    return converted("cwipc_hip_codec_inter_pack", out, capacity, errorMessage,
                     [&](auto &made) { return inter_pack((const uint8_t *)r, rlen, (const uint8_t *)p, plen, gop_index, made); });
}

extern "C" size_t cwipc_hip_codec_inter_unpack(const void *r, size_t rlen, const void *d, size_t dlen, void *out, size_t capacity, char **errorMessage) {
    return converted("cwipc_hip_codec_inter_unpack", out, capacity, errorMessage,
                     [&](auto &made) { return inter_unpack((const uint8_t *)r, rlen, (const uint8_t *)d, dlen, made); });
}

extern "C" int cwipc_hip_codec_inter_info(const void *bytes, size_t len, cwipc_hip_codec_inter_directory *info, char **errorMessage) {
    return info_of<InterLayout>("cwipc_hip_codec_inter_info", info, errorMessage, [&](InterLayout &e) { return inter_validate((const uint8_t *)bytes, len, nullptr, e); },
                                [&](const InterLayout &e) {
                                    info->kind = e.kind;
                                    info->gop_index = e.gop_index;
                                    info->ref_timestamp = e.ref_timestamp;
                                    info->ref_nleaves = e.ref_nleaves;
                                    info->embedded_entropy = e.embedded_entropy ? 1 : 0;
                                    info->nadded = e.nadded;
                                    for (int d = 0; d < e.cwao.bits; d++) info->nodes_added[d] = e.nodes_added[d];
                                    fill_directory(e, info, info->kind_of);
                                });
}

// ---- level-of-detail cuts of packets ----
extern "C" size_t cwipc_hip_codec_lod(const void *bytes, size_t len, int bits, void *out, size_t capacity, char **errorMessage) {
    return converted("cwipc_hip_codec_lod", out, capacity, errorMessage, [&](auto &made) { return lod_convert((const uint8_t *)bytes, len, bits, made); });
}
