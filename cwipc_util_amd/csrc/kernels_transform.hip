// kernels_transform.hip -- gfx950 kernels of transform colour coding (RULE T: hip_ext.h; the arithmetic: transform_terms.hpp).
//
// The tree.  Nodes are numbered across depths, so an inner node's number is the index of its occupancy byte and ONE exclusive scan
// of the popcounts of all occupancy bytes gives every inner node's first child (first[i] = 1 + the bits in front of byte i): three
// launches for the whole tree instead of three per depth.  A parent's first coefficient is first[i] - i - 1.  A leaf's weight is 1 and
// is not stored.
//
// Encode, on the body that codec_emit left on the device:  first[] -> the YCoCg planes of the leaves -> per depth from the deepest up,
// one lane per parent: its up to 8 children (contiguous numbers) and their weights, the at most 7 butterflies in registers, one
// value and one weight to the parent, k - 1 zigzag values to their places; the three channels are the grid's second dimension.  All
// depths whose parents fit one workgroup run in ONE launch of three workgroups, one a channel, a barrier between depths.  Then one
// count-scan-scatter over the coefficients for the escapes' places (their order is the coefficients': deterministic bytes), RULE E's
// stage on occupancy, tokens and tiles, and one kernel that puts the packet together around the escape streams, whose sizes only
// the device knows.
//
// Decode.  first[] -> the tokens' count-scan-scatter (the totals are the check of nescapes, fetched by the host in feed's one wait)
// -> weights from the deepest depth up -> values from the root down -> the colour plane that codec_points reads.
// Every load of a child is bounded by the tree's node count and every store by the header's counts, whatever the bytes.
#include "internal.hpp"
#include "block_scan.hpp"
#include "transform_terms.hpp"

namespace cwipc_amd {
namespace k {

static constexpr int TB = 256;   // lanes per workgroup, one node or coefficient each
static constexpr uint32_t NONE = 0xffffffffu;

static size_t tblocks(size_t n) { return (n + TB - 1) / TB; }
static size_t even(size_t words) { return (words + 1) & ~(size_t)1; }
// the scratch words: the first-child scan's counts and its sink; the escape scan's three rows of counts and their sinks
static size_t first_sink_at(const TransformTree &t) { return even(tblocks(t.inner) + 1); }
static size_t escape_counts_at(const TransformTree &t) { return first_sink_at(t) + 2; }
static size_t escape_row(const TransformTree &t) { return tblocks(t.nleaves - 1u) + 1; }
static size_t escape_sink_at(const TransformTree &t) { return even(escape_counts_at(t) + 3 * escape_row(t)); }
size_t transform_scan_words(const TransformTree &t) { return escape_sink_at(t) + 6 + 2; }
const uint32_t *transform_escape_total(const TransformTree &t, int ch) { return t.scan + escape_counts_at(t) + (size_t)(ch + 1) * escape_row(t) - 1; }

void transform_tree_counts(TransformTree &t, int bits, const uint32_t *nodes, uint32_t nleaves, uint32_t q16) {
    t.bits = bits;
    t.nleaves = nleaves;
    uint32_t at = 0;
    for (int L = 0; L < bits; L++) {
        t.depth_begin[L] = at;
        t.depth_count[L] = L == 0 ? 1u : nodes[L - 1];
        at += t.depth_count[L];
    }
    t.inner = at;
    for (int ch = 0; ch < 3; ch++) {
        t.q16[ch] = transform_channel_q16(q16, ch);
        t.leaf_step[ch] = transform_step(t.q16[ch], 1u, 1u);
    }
}

// ---------------------------------------------------------------------------
// the tree
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) transform_popcount_kernel(TransformTree t) {
    __shared__ uint32_t wave_tot[TB / 64];
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    const uint32_t v = block_sum<TB>(i < t.inner ? (uint32_t)__popc((unsigned)t.occupancy[i]) : 0u, wave_tot);
    if (threadIdx.x == 0) t.scan[blockIdx.x] = v;
}

__global__ void __launch_bounds__(TB) transform_first_scan_kernel(TransformTree t, size_t nblocks, size_t sink_at) {
    scan_block_counts<TB>(t.scan, nblocks, reinterpret_cast<unsigned long long *>(t.scan + sink_at), 0u);
}

__global__ void __launch_bounds__(TB) transform_first_kernel(TransformTree t) {
    __shared__ uint32_t wave_tot[TB / 64];
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    const uint32_t c = i < t.inner ? (uint32_t)__popc((unsigned)t.occupancy[i]) : 0u;
    const uint32_t before = block_exclusive_scan<TB>(c, wave_tot, nullptr);
    if (i < t.inner) t.first[i] = 1u + t.scan[blockIdx.x] + before;
}

// the numbers and weights of parent i's children by child place; NONE and 0 where there is none
__device__ __forceinline__ void children_of(const TransformTree &t, uint32_t i, uint32_t at[8], uint32_t w[8]) {
    const uint32_t byte = t.occupancy[i], first = t.first[i], total = t.inner + t.nleaves;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const uint32_t number = first + (uint32_t)__popc(byte & ((1u << c) - 1u));
        const bool present = ((byte >> c) & 1u) != 0u && number < total && number > i;
        at[c] = present ? number : NONE;
        w[c] = !present ? 0u : number >= t.inner ? 1u : t.weight[number];
    }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) transform_ycocg_kernel(TransformTree t, const uint8_t *__restrict__ colours) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j >= t.nleaves) return;
    const size_t total = (size_t)t.inner + t.nleaves;
    int32_t v[3];
    transform_to_ycocg(colours[3 * j], colours[3 * j + 1], colours[3 * j + 2], v);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) t.value[(size_t)ch * total + t.inner + j] = v[ch];
}

// one channel of parent i.  (Every channel writes the parent's weight, the same word: a channel's lanes read back only what lanes of
// their own channel wrote, which matters where the channels are workgroups of one launch.)
__device__ __forceinline__ void forward_parent(const TransformTree &t, uint32_t i, int ch) {
    uint32_t at[8], w[8], w1[7], w2[7];
    children_of(t, i, at, w);
    t.weight[i] = transform_places(w, w1, w2);
    const size_t total = (size_t)t.inner + t.nleaves, ncoef = (size_t)t.nleaves - 1u;
    const uint32_t coef0 = t.first[i] - i - 1u;
    {
        int32_t *plane = t.value + (size_t)ch * total;
        int64_t v[8], d[7];
#pragma unroll
        for (int c = 0; c < 8; c++) v[c] = at[c] != NONE ? (int64_t)plane[at[c]] : 0;
        plane[i] = (int32_t)transform_node_forward(w1, w2, v, d);
        uint32_t place = coef0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            if (!w1[k] || !w2[k]) continue;
            // (two leaves: the step is a constant of the launch, and transform_lift took its shift)
            const uint32_t step = w1[k] == 1u && w2[k] == 1u ? t.leaf_step[ch] : transform_step(t.q16[ch], w1[k], w2[k]);
            if (place < ncoef) t.zz[(size_t)ch * ncoef + place] = transform_zigzag(transform_quantise(d[k], step));
            place++;
        }
    }
}

__global__ void __launch_bounds__(TB) transform_forward_kernel(TransformTree t, uint32_t begin, uint32_t count) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p < count) forward_parent(t, begin + (uint32_t)p, (int)blockIdx.y);
}

// the depths top .. 0, whose parents fit one workgroup each: one launch, a workgroup a channel, its own stores read back behind a barrier
__global__ void __launch_bounds__(TB) transform_forward_top_kernel(TransformTree t, int top) {
    for (int L = top; L >= 0; L--) {
        if (threadIdx.x < t.depth_count[L]) forward_parent(t, t.depth_begin[L] + threadIdx.x, (int)blockIdx.x);
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// tokens and escapes: one count-scan-scatter over the coefficients, a row per channel
// ---------------------------------------------------------------------------
// tokens == nullptr: the encoder's, an escape is a zigzag value of 255 or more; otherwise the decoder's, a token equal to 255
__global__ void __launch_bounds__(TB) transform_escape_count_kernel(TransformTree t, const uint8_t *__restrict__ tokens, uint32_t *__restrict__ counts, size_t row) {
    __shared__ uint32_t wave_tot[TB / 64];
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x, ncoef = (size_t)t.nleaves - 1u, ch = blockIdx.y;
    uint32_t is = 0;
    if (j < ncoef) is = tokens ? (tokens[ch * ncoef + j] == 255u ? 1u : 0u) : (t.zz[ch * ncoef + j] >= 255u ? 1u : 0u);
    const uint32_t v = block_sum<TB>(is, wave_tot);
    if (threadIdx.x == 0) counts[ch * row + blockIdx.x] = v;
}

__global__ void __launch_bounds__(TB) transform_escape_scan_kernel(uint32_t *__restrict__ counts, size_t row, unsigned long long *__restrict__ totals, uint32_t tag) {
    scan_block_counts<TB>(counts + (size_t)blockIdx.x * row, row - 1, totals + blockIdx.x, tag);
}

__global__ void __launch_bounds__(TB) transform_tokens_kernel(TransformTree t, const uint32_t *__restrict__ counts, size_t row, uint8_t *__restrict__ tokens,
                                                            uint16_t *__restrict__ escapes, uint32_t escape_stride) {
    __shared__ uint32_t wave_tot[TB / 64];
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x, ncoef = (size_t)t.nleaves - 1u, ch = blockIdx.y;
    const uint32_t z = j < ncoef ? t.zz[ch * ncoef + j] : 0u;
    const uint32_t is = z >= 255u ? 1u : 0u;
    const uint32_t rank = counts[ch * row + blockIdx.x] + block_exclusive_scan<TB>(is, wave_tot, nullptr);
    if (j >= ncoef) return;
    tokens[ch * ncoef + j] = (uint8_t)(is ? 255u : z);
    if (is && rank < escape_stride) escapes[ch * escape_stride + rank] = (uint16_t)(z - 255u);
}

__global__ void __launch_bounds__(TB) transform_untoken_kernel(TransformTree t, const uint32_t *__restrict__ counts, size_t row, const uint8_t *__restrict__ tokens,
                                                             const uint8_t *__restrict__ in, uint32_t off0, uint32_t off1, uint32_t off2, uint32_t n0, uint32_t n1,
                                                             uint32_t n2) {
    __shared__ uint32_t wave_tot[TB / 64];
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x, ncoef = (size_t)t.nleaves - 1u, ch = blockIdx.y;
    const uint32_t token = j < ncoef ? tokens[ch * ncoef + j] : 0u;
    const uint32_t is = token == 255u ? 1u : 0u;
    const uint32_t rank = counts[ch * row + blockIdx.x] + block_exclusive_scan<TB>(is, wave_tot, nullptr);
    if (j >= ncoef) return;
    const uint32_t offset = ch == 0 ? off0 : ch == 1 ? off1 : off2, have = ch == 0 ? n0 : ch == 1 ? n1 : n2;
    uint32_t z = token;
    if (is && rank < have) z += (uint32_t)in[offset + 2u * rank] | ((uint32_t)in[offset + 2u * rank + 1u] << 8);   // (a rank past the stream: the host refuses the packet)
    t.zz[ch * ncoef + j] = z;
}

// ---------------------------------------------------------------------------
// the packet around the escape streams
// ---------------------------------------------------------------------------
__device__ __forceinline__ void copy_words(uint8_t *dst, const uint8_t *src, uint32_t bytes) {
    const uint32_t *from = reinterpret_cast<const uint32_t *>(src);
    uint32_t *to = reinterpret_cast<uint32_t *>(dst);
    for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < bytes / 4u; i += (size_t)gridDim.x * TB) to[i] = from[i];
}

// Every lane walks the (at most 23) streams and knows every offset; the copies are spread over the grid.  All sizes and offsets are
// multiples of 4.
__global__ void __launch_bounds__(TB) transform_assemble_kernel(TransformAssemble a) {
    const bool first_lane = blockIdx.x == 0 && threadIdx.x == 0;
    int S1 = a.entropy_streams;
    if (S1 > 0 && a.plan[3 * (S1 - 1)] > 1u) S1--;   // uniform tiles: the entropy stage left the tile plane out
    const int S = S1 + 3;
    bool fits = a.in_report[0] != 0u;
    uint64_t at = TRANSFORM_FIXED_BYTES + 4u + 8u * (uint64_t)S;
    int entry = 0;
    for (int s = 0; s < S1; s++) {
        const uint32_t mode = a.plan[3 * s], offset = a.plan[3 * s + 1], bytes = a.plan[3 * s + 2];
        const bool room = at + bytes <= a.out_capacity;
        if (room) copy_words(a.out + at, a.in + offset, bytes);
        if (first_lane && room) {
            uint32_t *e = reinterpret_cast<uint32_t *>(a.out + TRANSFORM_FIXED_BYTES + 4u + 8u * (size_t)entry);
            e[0] = mode;
            e[1] = bytes;
        }
        fits = fits && room;
        at += bytes;
        entry++;
        const int ch = s - a.bits;
        if (ch < 0 || ch > 2) continue;
        // behind a token stream its channel's escapes: u16 values, the padding the zeros the plane was filled with
        const uint32_t count = *a.escape_total[ch];
        const uint32_t raw = count <= a.escape_stride - 1u ? (2u * count + 3u) & ~3u : 0u;
        const bool room2 = at + raw <= a.out_capacity && count <= a.escape_stride - 1u;
        if (room2) copy_words(a.out + at, reinterpret_cast<const uint8_t *>(a.escapes + (size_t)ch * a.escape_stride), raw);
        if (first_lane && room2) {
            uint32_t *e = reinterpret_cast<uint32_t *>(a.out + TRANSFORM_FIXED_BYTES + 4u + 8u * (size_t)entry);
            e[0] = 0u;
            e[1] = raw;
        }
        fits = fits && room2;
        at += raw;
        entry++;
    }
    if (!first_lane) return;
    if (a.out_capacity >= TRANSFORM_FIXED_BYTES + 4u) {
        uint16_t *h = reinterpret_cast<uint16_t *>(a.out);
        h[0] = (uint16_t)a.q16;
        uint32_t *w = reinterpret_cast<uint32_t *>(a.out);
        for (int ch = 0; ch < 3; ch++) {
            h[1 + ch] = (uint16_t)(int16_t)*a.dc[ch];
            w[2 + ch] = *a.escape_total[ch];
        }
        w[5] = (uint32_t)S;
    }
    a.report[0] = (uint32_t)(fits && at <= a.out_capacity ? at : 0u);
    a.report[1] = (uint32_t)S;
    a.report[2] = a.in_report[2];
    a.report[3] = a.in_report[3];
}

// ---------------------------------------------------------------------------
// inverse
// ---------------------------------------------------------------------------
__device__ __forceinline__ void weigh_parent(const TransformTree &t, uint32_t i) {
    uint32_t at[8], w[8], sum = 0;
    children_of(t, i, at, w);
#pragma unroll
    for (int c = 0; c < 8; c++) sum += w[c];
    t.weight[i] = sum;
}

__global__ void __launch_bounds__(TB) transform_weights_kernel(TransformTree t, uint32_t begin, uint32_t count) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p < count) weigh_parent(t, begin + (uint32_t)p);
}

__device__ __forceinline__ void inverse_parent(const TransformTree &t, uint32_t i, int ch) {
    uint32_t at[8], w[8], w1[7], w2[7];
    children_of(t, i, at, w);
    transform_places(w, w1, w2);
    const size_t total = (size_t)t.inner + t.nleaves, ncoef = (size_t)t.nleaves - 1u;
    const uint32_t coef0 = t.first[i] - i - 1u;
    {
        int32_t *plane = t.value + (size_t)ch * total;
        int64_t v[8], d[7];
        uint32_t place = coef0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            d[k] = 0;
            if (!w1[k] || !w2[k]) continue;
            const uint32_t step = w1[k] == 1u && w2[k] == 1u ? t.leaf_step[ch] : transform_step(t.q16[ch], w1[k], w2[k]);
            if (place < ncoef) d[k] = transform_unzigzag(t.zz[(size_t)ch * ncoef + place]) * (int64_t)step;
            place++;
        }
        transform_node_inverse(w1, w2, (int64_t)plane[i], d, v);
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (at[c] != NONE) plane[at[c]] = (int32_t)v[c];
    }
}

__global__ void __launch_bounds__(TB) transform_inverse_kernel(TransformTree t, uint32_t begin, uint32_t count) {
    const size_t p = (size_t)blockIdx.x * TB + threadIdx.x;
    if (p < count) inverse_parent(t, begin + (uint32_t)p, (int)blockIdx.y);
}

// the depths 0 .. top in one launch, a workgroup a channel: the weights from `top` up (every workgroup makes them all, the same words),
// the root's value, then the values down to `top`'s children
__global__ void __launch_bounds__(TB) transform_inverse_top_kernel(TransformTree t, int top, int32_t dc0, int32_t dc1, int32_t dc2) {
    const int ch = (int)blockIdx.x;
    for (int L = top; L >= 0; L--) {
        if (threadIdx.x < t.depth_count[L]) weigh_parent(t, t.depth_begin[L] + threadIdx.x);
        __threadfence_block();
        __syncthreads();
    }
    if (threadIdx.x == 0) t.value[(size_t)ch * ((size_t)t.inner + t.nleaves)] = ch == 0 ? dc0 : ch == 1 ? dc1 : dc2;
    __threadfence_block();
    __syncthreads();
    for (int L = 0; L <= top; L++) {
        if (threadIdx.x < t.depth_count[L]) inverse_parent(t, t.depth_begin[L] + threadIdx.x, ch);
        __threadfence_block();
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TB) transform_rgb_kernel(TransformTree t, uint8_t *__restrict__ colours) {
    const size_t j = (size_t)blockIdx.x * TB + threadIdx.x;
    if (j >= t.nleaves) return;
    const size_t total = (size_t)t.inner + t.nleaves, at = (size_t)t.inner + j;
    const uint32_t c = transform_to_rgb(t.value[at], t.value[total + at], t.value[2 * total + at]);
    colours[3 * j] = (uint8_t)c;
    colours[3 * j + 1] = (uint8_t)(c >> 8);
    colours[3 * j + 2] = (uint8_t)(c >> 16);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// the deepest depth whose parents fit one workgroup (depth 0 has one)
static int top_depth(const TransformTree &t) {
    int top = 0;
    for (int L = 1; L < t.bits; L++)
        if (t.depth_count[L] <= (uint32_t)TB) top = L;
    return top;
}

void transform_prepare(const TransformTree &t, hipStream_t s) {
    const size_t nb = tblocks(t.inner);
    CW_LAUNCH("transform_popcount", transform_popcount_kernel, dim3((unsigned)nb), dim3(TB), 0, s, t);
    CW_LAUNCH("transform_first_scan", transform_first_scan_kernel, dim3(1), dim3(TB), 0, s, t, nb, first_sink_at(t));
    CW_LAUNCH("transform_first", transform_first_kernel, dim3((unsigned)nb), dim3(TB), 0, s, t);
}

void transform_forward(const TransformTree &t, const uint8_t *colours, hipStream_t s) {
    CW_LAUNCH("transform_ycocg", transform_ycocg_kernel, dim3((unsigned)tblocks(t.nleaves)), dim3(TB), 0, s, t, colours);
    const int top = top_depth(t);
    for (int L = t.bits - 1; L > top; L--)
        CW_LAUNCH("transform_forward", transform_forward_kernel, dim3((unsigned)tblocks(t.depth_count[L]), 3), dim3(TB), 0, s, t, t.depth_begin[L], t.depth_count[L]);
    CW_LAUNCH("transform_forward_top", transform_forward_top_kernel, dim3(3), dim3(TB), 0, s, t, top);
}

void transform_tokens(const TransformTree &t, uint8_t *tokens, uint16_t *escapes, uint32_t escape_stride, hipStream_t s) {
    const size_t row = escape_row(t), nb = row - 1;
    uint32_t *counts = t.scan + escape_counts_at(t);
    if (nb) CW_LAUNCH("transform_escape_count", transform_escape_count_kernel, dim3((unsigned)nb, 3), dim3(TB), 0, s, t, (const uint8_t *)nullptr, counts, row);
    CW_LAUNCH("transform_escape_scan", transform_escape_scan_kernel, dim3(3), dim3(TB), 0, s, counts, row, reinterpret_cast<unsigned long long *>(t.scan + escape_sink_at(t)), 0u);
    if (nb) CW_LAUNCH("transform_tokens", transform_tokens_kernel, dim3((unsigned)nb, 3), dim3(TB), 0, s, t, (const uint32_t *)counts, row, tokens, escapes, escape_stride);
}

void transform_assemble(const TransformAssemble &a, hipStream_t s) {
    CW_LAUNCH("transform_assemble", transform_assemble_kernel, dim3(64), dim3(TB), 0, s, a);
}

void transform_untoken(const TransformTree &t, const uint8_t *tokens, const uint8_t *in, const uint32_t escape_offset[3], const uint32_t nescapes[3],
                       unsigned long long *totals_host, uint32_t tag, hipStream_t s) {
    const size_t row = escape_row(t), nb = row - 1;
    uint32_t *counts = t.scan + escape_counts_at(t);
    if (nb) CW_LAUNCH("transform_escape_count", transform_escape_count_kernel, dim3((unsigned)nb, 3), dim3(TB), 0, s, t, tokens, counts, row);
    CW_LAUNCH("transform_escape_scan", transform_escape_scan_kernel, dim3(3), dim3(TB), 0, s, counts, row, totals_host, tag);
    if (nb)
        CW_LAUNCH("transform_untoken", transform_untoken_kernel, dim3((unsigned)nb, 3), dim3(TB), 0, s, t, (const uint32_t *)counts, row, tokens, in, escape_offset[0],
                  escape_offset[1], escape_offset[2], nescapes[0], nescapes[1], nescapes[2]);
}

void transform_inverse(const TransformTree &t, const int32_t dc[3], uint8_t *colours, hipStream_t s) {
    const int top = top_depth(t);
    for (int L = t.bits - 1; L > top; L--)
        CW_LAUNCH("transform_weights", transform_weights_kernel, dim3((unsigned)tblocks(t.depth_count[L])), dim3(TB), 0, s, t, t.depth_begin[L], t.depth_count[L]);
    CW_LAUNCH("transform_inverse_top", transform_inverse_top_kernel, dim3(3), dim3(TB), 0, s, t, top, dc[0], dc[1], dc[2]);
    for (int L = top + 1; L < t.bits; L++)
        CW_LAUNCH("transform_inverse", transform_inverse_kernel, dim3((unsigned)tblocks(t.depth_count[L]), 3), dim3(TB), 0, s, t, t.depth_begin[L], t.depth_count[L]);
    CW_LAUNCH("transform_rgb", transform_rgb_kernel, dim3((unsigned)tblocks(t.nleaves)), dim3(TB), 0, s, t, colours);
}

}  // namespace k
}  // namespace cwipc_amd
