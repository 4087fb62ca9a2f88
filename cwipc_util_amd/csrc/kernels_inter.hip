// kernels_inter.hip -- gfx950 kernels of inter-frame coding (RULE P: hip_ext.h; the arithmetic: inter_terms.hpp).
//
// Encode.  One wave after codec_cube decides between key and delta on the device (the frame's box against the GOP's cube) and leaves
// the cube the sort quantises in.  After codec_emit the frame's leaves are taken out of the packet body: keys compacted from the
// sorted points (the leaf starts, ranked by the scanned counts of the last depth), colours unpacked to a byte a channel, tiles copied.
// They are the next frame's reference.  Match: a lane per leaf of R searches P's keys (its ballot IS the keep byte stream: 64 lanes,
// 8 bytes), a lane per leaf of P searches R's keys for its predictor and writes the four residual bytes; both lists are in Morton
// order, so neighbouring lanes walk neighbouring paths of the search.  The leaves without a partner are compacted (count, scan,
// scatter); their node counts come from codec_count_scan and their occupancy bytes from an occupancy-only emit.
//
// Decode.  After the streams are decoded (kernels_entropy.hip) and A's keys expanded (codec_expand): the kept leaves are ranked (count,
// scan, rank), the checks run, and only for a delta that passed them the two sorted lists are merged by rank, the colours and tiles
// rebuilt and the points made.  Every store is bounded by the header's counts, for any payload bytes.
#include "internal.hpp"
#include "block_scan.hpp"
#include "inter_terms.hpp"

namespace cwipc_amd {
namespace k {

static constexpr int IB = 256;           // lanes per workgroup, one leaf each (codec_count_scan's CB: the offsets are per 256 keys)
static constexpr int IWAVES = IB / 64;

static unsigned inter_blocks(size_t n) { return (unsigned)((n + IB - 1) / IB); }

// ---------------------------------------------------------------------------
// encode: key or delta, and the cube
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) inter_cube_kernel(const CodecBounds *__restrict__ partial, unsigned nb, InterCubeReport *__restrict__ report, int allow_delta,
                                                       float gx, float gy, float gz, double gop_side, float exp_factor) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (unsigned i = threadIdx.x; i < nb; i += 64) {
        const CodecBounds b = partial[i];
        if (!b.count) continue;
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], b.lo[a]); hi[a] = fmaxf(hi[a], b.hi[a]); }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; a++) {   // (a step folds the box)
            lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64));
        }
    if (threadIdx.x != 0) return;
    CodecCube c = report->cube;
    uint32_t delta = 0;
    if (c.nfinite) {
        const float gop_mn[3] = {gx, gy, gz};
        if (allow_delta && inter_contained(lo, hi, gop_mn, gop_side)) {
            for (int a = 0; a < 3; a++) c.mn[a] = gop_mn[a];
            c.side = gop_side;
            delta = 1;
        } else {
            float mn[3];
            double side;
            inter_expand_cube(c.mn, c.side, exp_factor, mn, side);
            for (int a = 0; a < 3; a++) c.mn[a] = mn[a];
            c.side = side;
        }
    }
    report->cube = c;
    report->delta = delta;
    report->pad = 0;
}

void inter_cube(const void *partial, size_t npoints, InterCubeReport *report, bool allow_delta, const float gop_mn[3], double gop_side, float exp_factor,
                hipStream_t s) {
    size_t nb = (npoints + IB - 1) / IB;   // codec_cube's grid
    nb = nb > 512 ? 512 : nb;
    CW_LAUNCH("inter_cube", inter_cube_kernel, dim3(1), dim3(64), 0, s, (const CodecBounds *)partial, (unsigned)nb, report, allow_delta ? 1 : 0, gop_mn[0], gop_mn[1],
              gop_mn[2], gop_side, exp_factor);
}

// ---------------------------------------------------------------------------
// a frame's leaves out of a packet body
// ---------------------------------------------------------------------------
// sorted point i starts a leaf iff its key differs from its predecessor's; its leaf index is the number of starts up to it, less one:
// the scanned counts of the last depth (row e.bits - 1 of codec_count_scan's table) plus the starts of this workgroup in front of it
__global__ void __launch_bounds__(IB) inter_leaf_keys_kernel(const unsigned long long *__restrict__ keys, const CodecCube *__restrict__ cube,
                                                            const uint32_t *__restrict__ offsets, uint32_t nleaves, unsigned long long *__restrict__ out) {
    __shared__ uint32_t wave_lds[IWAVES];
    const size_t i = (size_t)blockIdx.x * IB + threadIdx.x;
    const bool valid = i < (size_t)cube->nfinite;
    const unsigned long long key = valid ? keys[i] : 0ull;
    const bool start = valid && (i == 0 || keys[i - 1] != key);
    const uint32_t before = block_exclusive_scan<IB>(start ? 1u : 0u, wave_lds, nullptr);
    const uint32_t leaf = offsets[blockIdx.x] + before;
    if (start && leaf < nleaves) out[leaf] = key;
}

// leaf j: its three stored colours out of the bit-packed plane, a byte each; its tile
__global__ void __launch_bounds__(IB) inter_unpack_kernel(const uint32_t *__restrict__ colours, uint64_t colour_words, const uint8_t *__restrict__ tiles, int tile_value,
                                                         int cb, InterLeavesDev out) {
    const size_t j = (size_t)blockIdx.x * IB + threadIdx.x;
    if (j >= out.n) return;
    const uint64_t bit = (uint64_t)j * (uint64_t)(3 * cb);
    const uint64_t word = bit >> 5;
    const uint32_t off = (uint32_t)(bit & 31u);
    uint32_t packed = word < colour_words ? colours[word] >> off : 0u;
    if (off + 3u * (uint32_t)cb > 32u && word + 1 < colour_words) packed |= colours[word + 1] << (32u - off);
    const uint32_t mask = (1u << cb) - 1u;
    out.colour[j] = (uint8_t)(packed & mask);
    out.colour[(size_t)out.n + j] = (uint8_t)((packed >> cb) & mask);
    out.colour[2 * (size_t)out.n + j] = (uint8_t)((packed >> (2 * cb)) & mask);
    out.tiles[j] = tiles ? tiles[j] : (uint8_t)tile_value;
}

void inter_leaves_of_planes(const uint32_t *colours, uint64_t colour_words, const uint8_t *tiles, int tile_value, int colour_bits, const InterLeavesDev &out,
                            hipStream_t s) {
    if (!out.n) return;
    CW_LAUNCH("inter_unpack", inter_unpack_kernel, dim3(inter_blocks(out.n)), dim3(IB), 0, s, colours, colour_words, tiles, tile_value, colour_bits, out);
}

void inter_leaves_of_body(const unsigned long long *sorted_keys, size_t npoints, const CodecCube *cube, const uint32_t *offsets, const CodecEmit &e,
                          int colour_bits, const InterLeavesDev &out, hipStream_t s) {
    if (!out.n || !npoints) return;
    const size_t nb = codec_blocks(npoints);
    CW_LAUNCH("inter_leaf_keys", inter_leaf_keys_kernel, dim3((unsigned)nb), dim3(IB), 0, s, sorted_keys, cube, offsets + (size_t)(e.bits - 1) * (nb + 1), out.n,
              out.keys);
    inter_leaves_of_planes(e.colours, e.colour_words, e.tiles, 0, colour_bits, out, s);
}

// ---------------------------------------------------------------------------
// encode: match
// ---------------------------------------------------------------------------
// a lane per leaf of R: is it a leaf of P?  The ballot of a wave is eight keep bytes; lanes past R.n vote 0, the padding bits.
__global__ void __launch_bounds__(IB) inter_keep_kernel(InterLeavesDev R, InterLeavesDev P, uint8_t *__restrict__ keep) {
    const size_t i = (size_t)blockIdx.x * IB + threadIdx.x;
    bool found = false;
    if (i < R.n) (void)inter_predictor(P.keys, P.n, R.keys[i], found);
    const unsigned long long b = __ballot(found);
    const uint32_t lane = threadIdx.x & 63u;
    const size_t byte = (i - lane) / 8u + lane;
    if (lane < 8u && byte < ((size_t)R.n + 7u) / 8u) keep[byte] = (uint8_t)(b >> (8u * lane));
}

// a lane per leaf of P: its predictor in R, the four residual bytes, whether it is new; the new ones counted per workgroup
__global__ void __launch_bounds__(IB) inter_residual_kernel(InterLeavesDev R, InterLeavesDev P, int cb, uint8_t *__restrict__ res, uint8_t *__restrict__ is_added,
                                                           uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_lds[IWAVES];
    const size_t j = (size_t)blockIdx.x * IB + threadIdx.x;
    uint32_t added = 0;
    if (j < P.n) {
        bool found = false;
        const uint32_t pred = inter_predictor(R.keys, R.n, P.keys[j], found);
        for (uint32_t ch = 0; ch < 3u; ch++)
            res[(size_t)ch * P.n + j] = (uint8_t)inter_colour_symbol(P.colour[(size_t)ch * P.n + j], R.colour[(size_t)ch * R.n + pred], cb);
        res[3 * (size_t)P.n + j] = (uint8_t)(P.tiles[j] ^ R.tiles[pred]);
        added = found ? 0u : 1u;
        is_added[j] = (uint8_t)added;
    }
    const uint32_t total = block_sum<IB>(added, wave_lds);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(IB) inter_scan_kernel(uint32_t *__restrict__ counts, size_t nblocks, unsigned long long *__restrict__ total_host, uint32_t tag) {
    scan_block_counts<IB>(counts, nblocks, total_host, tag);
}

__global__ void __launch_bounds__(IB) inter_scatter_kernel(InterLeavesDev P, const uint8_t *__restrict__ is_added, const uint32_t *__restrict__ counts, size_t nblocks,
                                                          unsigned long long *__restrict__ added, CodecCube *__restrict__ cube_added) {
    __shared__ uint32_t wave_lds[IWAVES];
    const size_t j = (size_t)blockIdx.x * IB + threadIdx.x;
    const uint32_t mine = j < P.n ? is_added[j] : 0u;
    const uint32_t at = counts[blockIdx.x] + block_exclusive_scan<IB>(mine, wave_lds, nullptr);
    if (mine && at < P.n) added[at] = P.keys[j];
    if (j == 0) {   // what codec_count_kernel reads of a cube: how many keys take part
        CodecCube c{{0.f, 0.f, 0.f}, counts[nblocks], 1.0};
        *cube_added = c;
    }
}

void inter_match(const InterLeavesDev &R, const InterLeavesDev &P, int colour_bits, uint8_t *keep, uint8_t *res, unsigned long long *added, uint32_t *counts,
                 CodecCube *cube_added, unsigned long long *total_host, uint32_t tag, hipStream_t s) {
    const size_t nb = inter_blocks(P.n);
    uint8_t *is_added = reinterpret_cast<uint8_t *>(added) + 8u * (size_t)P.n;   // (the caller's block: P.n bytes behind the keys)
    CW_LAUNCH("inter_keep", inter_keep_kernel, dim3(inter_blocks(R.n)), dim3(IB), 0, s, R, P, keep);
    CW_LAUNCH("inter_residual", inter_residual_kernel, dim3((unsigned)nb), dim3(IB), 0, s, R, P, colour_bits, res, is_added, counts);
    CW_LAUNCH("inter_scan", inter_scan_kernel, dim3(1), dim3(IB), 0, s, counts, nb, total_host, tag);
    CW_LAUNCH("inter_scatter", inter_scatter_kernel, dim3((unsigned)nb), dim3(IB), 0, s, P, is_added, counts, nb, added, cube_added);
}

// ---------------------------------------------------------------------------
// encode: the occupancy bytes of the added leaves
// ---------------------------------------------------------------------------
// codec_emit_kernel's first half on keys that are distinct: key i starts a node at every depth from the first triple in which it
// differs from its predecessor; its node index at depth L is the number of starts at L up to it, less one
struct DepthOffsets {
    uint64_t at[CODEC_MAX_BITS];
};

__global__ void __launch_bounds__(IB) inter_occupancy_kernel(const unsigned long long *__restrict__ keys, uint32_t n, int bits, const uint32_t *__restrict__ offsets,
                                                            size_t nblocks, DepthOffsets depth, uint64_t occupancy_bytes, uint32_t *__restrict__ occupancy) {
    __shared__ uint32_t wave_tot[CODEC_MAX_BITS][IWAVES];
    const size_t i = (size_t)blockIdx.x * IB + threadIdx.x;
    const bool valid = i < (size_t)n;
    const unsigned long long key = valid ? keys[i] : 0ull;
    int t = bits;
    if (valid && i == 0) t = 0;
    if (valid && i > 0) t = (bits - 1) - (63 - __clzll((long long)(key ^ keys[i - 1]))) / 3;   // (the keys are distinct cells: the difference is below 3 * bits)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    uint32_t rank[CODEC_MAX_BITS];
#pragma unroll
    for (int L = 0; L < CODEC_MAX_BITS; L++) {
        rank[L] = 0;
        if (L < bits) {
            const unsigned long long b = __ballot(L >= t);
            rank[L] = (uint32_t)__popcll(b & upto);
            if (lane == 0) wave_tot[L][wave] = (uint32_t)__popcll(b);
        }
    }
    __syncthreads();
    if (!valid) return;
    uint32_t parent = 0;
#pragma unroll
    for (int L = 0; L < CODEC_MAX_BITS; L++) {
        if (L < bits) {
            uint32_t r = offsets[(size_t)L * (nblocks + 1) + blockIdx.x] + rank[L];
            for (int w = 0; w < wave; w++) r += wave_tot[L][w];
            if (L >= t) {
                const uint64_t byte = depth.at[L] + (uint64_t)parent;
                const uint32_t child = (uint32_t)(key >> (3 * (bits - 1 - L))) & 7u;
                if (byte < occupancy_bytes) atomicOr(&occupancy[byte >> 2], 1u << (8u * (uint32_t)(byte & 3u) + child));
            }
            parent = r - 1u;
        }
    }
}

void inter_occupancy(const unsigned long long *keys, uint32_t n, size_t grid_n, int bits, const uint32_t *offsets, const uint64_t depth_offset[16],
                     uint64_t occupancy_bytes, uint32_t *occupancy, hipStream_t s) {
    if (!n) return;
    DepthOffsets depth;
    for (int L = 0; L < CODEC_MAX_BITS; L++) depth.at[L] = depth_offset[L];
    CW_LAUNCH("inter_occupancy", inter_occupancy_kernel, dim3(inter_blocks(n)), dim3(IB), 0, s, keys, n, bits, offsets, codec_blocks(grid_n), depth, occupancy_bytes,
              occupancy);
}

// ---------------------------------------------------------------------------
// decode: the checks
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t keep_bit(const uint8_t *__restrict__ keep, size_t i) { return ((uint32_t)keep[i >> 3] >> (uint32_t)(i & 7u)) & 1u; }

__global__ void __launch_bounds__(IB) inter_keep_count_kernel(const uint8_t *__restrict__ keep, uint32_t nr, uint32_t *__restrict__ counts, uint32_t *__restrict__ flags) {
    __shared__ uint32_t wave_lds[IWAVES];
    const size_t i = (size_t)blockIdx.x * IB + threadIdx.x;
    const uint32_t total = block_sum<IB>(i < nr ? keep_bit(keep, i) : 0u, wave_lds);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
    if (i == 0 && (nr & 7u) && ((uint32_t)keep[nr >> 3] >> (nr & 7u))) atomicOr(flags, 16u);
}

// rank[i]: the kept leaves of R in front of leaf i; rank[nr]: all of them
__global__ void __launch_bounds__(IB) inter_keep_rank_kernel(const uint8_t *__restrict__ keep, uint32_t nr, const uint32_t *__restrict__ counts, uint32_t *__restrict__ rank) {
    __shared__ uint32_t wave_lds[IWAVES];
    const size_t i = (size_t)blockIdx.x * IB + threadIdx.x;
    const uint32_t mine = i < nr ? keep_bit(keep, i) : 0u;
    const uint32_t before = counts[blockIdx.x] + block_exclusive_scan<IB>(mine, wave_lds, nullptr);
    if (i < nr) rank[i] = before;
    if (i + 1 == nr) rank[nr] = before + mine;
}

__global__ void __launch_bounds__(IB) inter_overlap_kernel(InterLeavesDev R, const unsigned long long *__restrict__ added, uint32_t nadded, uint32_t *__restrict__ flags) {
    const size_t a = (size_t)blockIdx.x * IB + threadIdx.x;
    bool found = false;
    if (a < nadded) (void)inter_predictor(R.keys, R.n, added[a], found);
    if (__any(found) && (threadIdx.x & 63) == 0) atomicOr(flags, 8u);
}

__global__ void __launch_bounds__(64) inter_status_kernel(const uint32_t *__restrict__ counts, size_t nblocks, uint32_t nadded, uint32_t nleaves,
                                                         const uint32_t *__restrict__ flags, unsigned long long *__restrict__ status_host, uint32_t tag) {
    if (threadIdx.x != 0) return;
    uint32_t status = flags[0];
    if ((uint64_t)counts[nblocks] + nadded != nleaves) status |= 32u;
    __hip_atomic_store(status_host, ((unsigned long long)tag << 32) | status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

void inter_check(const InterLeavesDev &R, const uint8_t *keep, const unsigned long long *added, uint32_t nadded, uint32_t nleaves, uint32_t *rank,
                 uint32_t *counts, uint32_t *flags, unsigned long long *status_host, uint32_t tag, hipStream_t s) {
    const size_t nb = inter_blocks(R.n);
    CW_LAUNCH("inter_keep_count", inter_keep_count_kernel, dim3((unsigned)nb), dim3(IB), 0, s, keep, R.n, counts, flags);
    CW_LAUNCH("inter_scan", inter_scan_kernel, dim3(1), dim3(IB), 0, s, counts, nb, status_host + 1, tag);
    CW_LAUNCH("inter_keep_rank", inter_keep_rank_kernel, dim3((unsigned)nb), dim3(IB), 0, s, keep, R.n, counts, rank);
    if (nadded) CW_LAUNCH("inter_overlap", inter_overlap_kernel, dim3(inter_blocks(nadded)), dim3(IB), 0, s, R, added, nadded, flags);
    CW_LAUNCH("inter_status", inter_status_kernel, dim3(1), dim3(64), 0, s, counts, nb, nadded, nleaves, flags, status_host, tag);
}

// ---------------------------------------------------------------------------
// decode: the frame a delta stands for
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lower_bound(const unsigned long long *__restrict__ keys, uint32_t n, unsigned long long k) {
    uint32_t lo = 0, hi = n;   // the number of keys < k
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (keys[mid] < k) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// lanes 0 .. R.n - 1: a kept leaf of R goes behind the kept ones in front of it and the added ones below it; lanes R.n ..: an added
// leaf goes behind the added ones in front of it and the kept ones below it.  The checks have held the two lists apart.
__global__ void __launch_bounds__(IB) inter_merge_kernel(InterLeavesDev R, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ rank,
                                                        const unsigned long long *__restrict__ added, uint32_t nadded, InterLeavesDev P) {
    const size_t i = (size_t)blockIdx.x * IB + threadIdx.x;
    if (i < R.n) {
        if (!keep_bit(keep, i)) return;
        const unsigned long long key = R.keys[i];
        const size_t at = (size_t)rank[i] + lower_bound(added, nadded, key);
        if (at < P.n) P.keys[at] = key;
    } else if (i - R.n < nadded) {
        const size_t a = i - R.n;
        const unsigned long long key = added[a];
        const size_t at = a + rank[lower_bound(R.keys, R.n, key)];
        if (at < P.n) P.keys[at] = key;
    }
}

__global__ void __launch_bounds__(IB) inter_rebuild_kernel(InterLeavesDev R, const uint8_t *__restrict__ res, CodecDecode d, int tile_mode, InterLeavesDev P,
                                                          float *__restrict__ ox, float *__restrict__ oy, float *__restrict__ oz, uint32_t *__restrict__ ow) {
    const size_t j = (size_t)blockIdx.x * IB + threadIdx.x;
    if (j >= P.n) return;
    const unsigned long long key = P.keys[j];
    bool found = false;
    const uint32_t pred = inter_predictor(R.keys, R.n, key, found);
    const int cb = d.colour_bits, shift = 8 - cb;
    uint32_t v[3];
    for (uint32_t ch = 0; ch < 3u; ch++) {
        v[ch] = inter_colour_value(R.colour[(size_t)ch * R.n + pred], res[(size_t)ch * P.n + j], cb);
        P.colour[(size_t)ch * P.n + j] = (uint8_t)v[ch];
    }
    const uint32_t tile = tile_mode == 1 ? (uint32_t)(R.tiles[pred] ^ res[3 * (size_t)P.n + j]) : (uint32_t)d.tile_value;
    P.tiles[j] = (uint8_t)tile;
    uint32_t q[3];
    codec_unkey(key, q);
    ox[j] = codec_position(d.mn[0], q[0], d.cell);
    oy[j] = codec_position(d.mn[1], q[1], d.cell);
    oz[j] = codec_position(d.mn[2], q[2], d.cell);
    ow[j] = codec_colour_load(v[0], shift) | (codec_colour_load(v[1], shift) << 8) | (codec_colour_load(v[2], shift) << 16) | (tile << 24);
}

void inter_apply(const InterLeavesDev &R, const uint8_t *keep, const uint32_t *rank, const unsigned long long *added, uint32_t nadded, const uint8_t *res,
                 const CodecDecode &d, int tile_mode, const InterLeavesDev &P, const DeviceSoA &dst, hipStream_t s) {
    CW_LAUNCH("inter_merge", inter_merge_kernel, dim3(inter_blocks((size_t)R.n + nadded)), dim3(IB), 0, s, R, keep, rank, added, nadded, P);
    CW_LAUNCH("inter_rebuild", inter_rebuild_kernel, dim3(inter_blocks(P.n)), dim3(IB), 0, s, R, res, d, tile_mode, P, dst.x(), dst.y(), dst.z(), dst.rgbt());
}

}  // namespace k
}  // namespace cwipc_amd
