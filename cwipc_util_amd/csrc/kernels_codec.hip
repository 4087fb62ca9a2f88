// kernels_codec.hip -- gfx950 kernels of the octree codec (RULE C: hip_ext.h; the arithmetic: codec_terms.hpp).
//
// Encode.  bounds of the finite points -> cube -> keys (a point that is left out gets the key 1 << 3B, above every cell) -> stable
// radix sort of (key, index) over 3B + 1 bits -> per sorted point the shallowest triple in which its key differs from its
// predecessor's: from that depth on it starts a node.  Counting those starts per workgroup and depth and scanning the counts gives
// nodes[] (the one read-back) and every point's node index at every depth: the emit kernel ORs the occupancy bits and adds the
// colours into per-leaf sums (integer, hence order-free), the leaf kernel rounds, packs and writes the tile bytes.  An encoder with
// fewer bits than the sort was made for reads the same keys and the same counts: depth L of a B-bit key is depth L of its b-bit prefix.
//
// Decode.  Per depth: popcount per node, scan, expand the child prefixes; then leaves -> points.  The packet has passed
// codec_validate() on the host before any of this is launched; every store is bounded by the header's counts all the same.
#include "internal.hpp"
#include "block_scan.hpp"
#include "codec_terms.hpp"

#include <rocprim/device/device_radix_sort.hpp>

namespace cwipc_amd {
namespace k {

static constexpr int CB = 256;           // lanes per workgroup, one point or node each
static constexpr int CWAVES = CB / 64;

size_t codec_blocks(size_t n) { return (n + CB - 1) / CB; }
static unsigned bounds_grid(size_t n) {
    size_t g = codec_blocks(n);
    return (unsigned)(g < 1 ? 1 : g > 512 ? 512 : g);
}

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ---------------------------------------------------------------------------
// encode: cube
// ---------------------------------------------------------------------------
using BoundsPartial = CodecBounds;

__global__ void __launch_bounds__(CB) codec_bounds_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                         BoundsPartial *__restrict__ partial) {
    __shared__ float red[6][CWAVES];
    __shared__ uint32_t cnt[CWAVES];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t count = 0;
    for (size_t i = (size_t)blockIdx.x * CB + threadIdx.x; i < n; i += (size_t)gridDim.x * CB) {
        const float p[3] = {x[i], y[i], z[i]};
        if (!(finite_bits(p[0]) && finite_bits(p[1]) && finite_bits(p[2]))) continue;
        count++;
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
    }
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64));
        }
        count += __shfl_down(count, off, 64);   // (a step folds the box and the count)
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; a++) { red[a][wave] = lo[a]; red[3 + a][wave] = hi[a]; }
        cnt[wave] = count;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        BoundsPartial b;
        for (int a = 0; a < 3; a++) { b.lo[a] = red[a][0]; b.hi[a] = red[3 + a][0]; }
        b.count = cnt[0];
        b.pad = 0;
        for (int w = 1; w < CWAVES; w++) {
            for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], red[a][w]); b.hi[a] = fmaxf(b.hi[a], red[3 + a][w]); }
            b.count += cnt[w];
        }
        partial[blockIdx.x] = b;
    }
}

// one wave: the partials (at most 512) into the cube
__global__ void __launch_bounds__(64) codec_cube_kernel(const BoundsPartial *__restrict__ partial, unsigned nb, CodecCube *__restrict__ cube) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t count = 0;
    for (unsigned i = threadIdx.x; i < nb; i += 64) {
        const BoundsPartial b = partial[i];
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], b.lo[a]); hi[a] = fmaxf(hi[a], b.hi[a]); }
        count += b.count;
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64));
        }
        count += __shfl_down(count, off, 64);   // (a step folds the box and the count)
    }
    if (threadIdx.x == 0) {
        CodecCube c;
        c.nfinite = count;
        if (count) {
            for (int a = 0; a < 3; a++) c.mn[a] = codec_min_canonical(lo[a]);
            c.side = codec_side(c.mn, hi);
        } else {
            c.mn[0] = c.mn[1] = c.mn[2] = 0.f;
            c.side = 1.0;
        }
        *cube = c;
    }
}

// ---------------------------------------------------------------------------
// encode: keys
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(CB) codec_keys_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                       const CodecCube *__restrict__ cube, int bits, unsigned long long *__restrict__ keys,
                                                       uint32_t *__restrict__ index) {
    const size_t i = (size_t)blockIdx.x * CB + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {x[i], y[i], z[i]};
    unsigned long long key = 1ull << (3 * bits);
    if (finite_bits(p[0]) && finite_bits(p[1]) && finite_bits(p[2])) {
        const double side = cube->side;
        key = codec_key(codec_cell(p[0], cube->mn[0], side, bits), codec_cell(p[1], cube->mn[1], side, bits), codec_cell(p[2], cube->mn[2], side, bits));
    }
    keys[i] = key;
    index[i] = (uint32_t)i;
}

// The depth from which sorted point i starts a node: 0 for the first point, `bits` (none) for a key equal to its predecessor's.
__device__ __forceinline__ int start_depth(const unsigned long long *__restrict__ keys, size_t i, unsigned long long key, int bits) {
    if (i == 0) return 0;
    const unsigned long long diff = key ^ keys[i - 1];
    if (diff == 0ull) return bits;
    const int high = 63 - __clzll((long long)diff);   // < 3 * bits: both keys are cells
    return (bits - 1) - high / 3;
}

// counts[L * (nblocks + 1) + b] = points of workgroup b that start a node at depth L, L < bits
__global__ void __launch_bounds__(CB) codec_count_kernel(const unsigned long long *__restrict__ keys, const CodecCube *__restrict__ cube, int bits,
                                                        uint32_t *__restrict__ counts, size_t nblocks) {
    __shared__ uint32_t wave_tot[CODEC_MAX_BITS][CWAVES];
    const size_t i = (size_t)blockIdx.x * CB + threadIdx.x;
    const bool valid = i < (size_t)cube->nfinite;
    const int t = valid ? start_depth(keys, i, keys[i], bits) : bits;
    const int wave = threadIdx.x >> 6;
    for (int L = 0; L < bits; L++) {
        const unsigned long long b = __ballot(L >= t);
        if ((threadIdx.x & 63) == 0) wave_tot[L][wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x < bits) {
        uint32_t v = 0;
        for (int w = 0; w < CWAVES; w++) v += wave_tot[threadIdx.x][w];
        counts[(size_t)threadIdx.x * (nblocks + 1) + blockIdx.x] = v;
    }
}

// workgroup L: the exclusive scan of depth L's counts; the total, nodes[L], behind them and into the pinned word L
__global__ void __launch_bounds__(CB) codec_scan_kernel(uint32_t *__restrict__ counts, size_t nblocks, unsigned long long *__restrict__ total_host, uint32_t tag) {
    scan_block_counts<CB>(counts + (size_t)blockIdx.x * (nblocks + 1), nblocks, total_host + blockIdx.x, tag);
}

// ---------------------------------------------------------------------------
// encode: occupancy bits and leaf sums
// ---------------------------------------------------------------------------
// sort_bits: what the keys were made for; e.bits <= sort_bits: what this packet holds.  Depth L of the two is the same triple.
__global__ void __launch_bounds__(CB) codec_emit_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ index,
                                                       const uint32_t *__restrict__ rgbt, const CodecCube *__restrict__ cube, int sort_bits,
                                                       const uint32_t *__restrict__ offsets, size_t nblocks, CodecEmit e) {
    __shared__ uint32_t wave_tot[CODEC_MAX_BITS][CWAVES];
    const size_t i = (size_t)blockIdx.x * CB + threadIdx.x;
    const bool valid = i < (size_t)cube->nfinite;
    const unsigned long long key = valid ? keys[i] : 0ull;
    const int t = valid ? start_depth(keys, i, key, sort_bits) : sort_bits;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    uint32_t rank[CODEC_MAX_BITS];   // the number of starts at depth L up to and including this point, in this wave
#pragma unroll
    for (int L = 0; L < CODEC_MAX_BITS; L++) {
        rank[L] = 0;
        if (L < e.bits) {
            const unsigned long long b = __ballot(L >= t);
            rank[L] = (uint32_t)__popcll(b & upto);
            if (lane == 0) wave_tot[L][wave] = (uint32_t)__popcll(b);
        }
    }
    __syncthreads();
    uint32_t leaf = 0xffffffffu;
    if (valid) {
        uint32_t parent = 0;   // the index, within its depth, of the node this point lies in
#pragma unroll
        for (int L = 0; L < CODEC_MAX_BITS; L++) {
            if (L < e.bits) {
                uint32_t r = offsets[(size_t)L * (nblocks + 1) + blockIdx.x] + rank[L];
                for (int w = 0; w < wave; w++) r += wave_tot[L][w];
                if (L >= t) {
                    const uint64_t byte = e.depth_offset[L] + (uint64_t)parent;
                    const uint32_t child = (uint32_t)(key >> (3 * (sort_bits - 1 - L))) & 7u;
                    if (byte < e.occupancy_bytes) atomicOr(&e.occupancy[byte >> 2], 1u << (8u * (uint32_t)(byte & 3u) + child));
                }
                parent = r - 1u;   // (r >= 1: the first point starts a node at every depth)
            }
        }
        leaf = parent;
    }
    // the colours and tiles of a leaf's points in this wave are added up here and reach memory once: a leaf of thousands of points costs
    // an atomic per wave, not per point
    const uint32_t w = valid ? rgbt[index[i]] : 0u;
    uint32_t rg = (w & 0xffu) | ((w & 0xff00u) << 8), bc = ((w >> 16) & 0xffu) | (1u << 16), tl = w >> 24;   // r | g << 16,  b | count << 16
    if (!valid) { rg = 0; bc = 0; tl = 0; }
    for (int off = 1; off < 64; off <<= 1) {   // (a segmented scan: four values a step, added only within a leaf)
        const uint32_t o_leaf = __shfl_up(leaf, off, 64), o_rg = __shfl_up(rg, off, 64), o_bc = __shfl_up(bc, off, 64), o_tl = __shfl_up(tl, off, 64);
        if (lane >= off && o_leaf == leaf) { rg += o_rg; bc += o_bc; tl |= o_tl; }
    }
    const uint32_t next_leaf = __shfl_down(leaf, 1, 64);
    if (valid && leaf < e.nleaves && (lane == 63 || next_leaf != leaf)) {
        CodecLeafSum *s = e.sums + leaf;
        atomicAdd(&s->r, (unsigned long long)(rg & 0xffffu));
        atomicAdd(&s->g, (unsigned long long)(rg >> 16));
        atomicAdd(&s->b, (unsigned long long)(bc & 0xffffu));
        atomicAdd(&s->count, bc >> 16);
        atomicOr(&s->tile, tl);
    }
}

// per leaf: the rounded means, shifted and packed; the tile byte; whether every leaf has the same tile (tile_stats[0] |= tile,
// tile_stats[1] |= ~tile & 255: uniform iff the two have no bit in common)
__global__ void __launch_bounds__(CB) codec_leaf_kernel(CodecEmit e, int shift) {
    const size_t j = (size_t)blockIdx.x * CB + threadIdx.x;
    uint32_t has = 0, lacks = 0;
    if (j < e.nleaves) {
        const CodecLeafSum s = e.sums[j];
        if (s.count) {
            const int cb = 8 - shift;
            const uint32_t packed = codec_colour_store(codec_leaf_mean(s.r, s.count), shift) | (codec_colour_store(codec_leaf_mean(s.g, s.count), shift) << cb) |
                                    (codec_colour_store(codec_leaf_mean(s.b, s.count), shift) << (2 * cb));
            const uint64_t bit = (uint64_t)j * (uint64_t)(3 * cb);
            const uint64_t word = bit >> 5;
            const uint32_t off = (uint32_t)(bit & 31u);
            if (word < e.colour_words) atomicOr(&e.colours[word], packed << off);
            if (off + 3u * (uint32_t)cb > 32u && word + 1 < e.colour_words) atomicOr(&e.colours[word + 1], packed >> (32u - off));
        }
        e.tiles[j] = (uint8_t)s.tile;
        has = s.tile & 255u;
        lacks = ~s.tile & 255u;
    }
    for (int off = 32; off > 0; off >>= 1) {
        has |= __shfl_down(has, off, 64);
        lacks |= __shfl_down(lacks, off, 64);
    }
    // (the two words only ever gain bits: a wave that has nothing to add -- nearly every wave after the first few -- leaves them alone)
    if ((threadIdx.x & 63) == 0) {
        if (has & ~__hip_atomic_load(&e.tile_stats[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&e.tile_stats[0], has);
        if (lacks & ~__hip_atomic_load(&e.tile_stats[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&e.tile_stats[1], lacks);
    }
}

// ---------------------------------------------------------------------------
// encode: launchers
// ---------------------------------------------------------------------------
size_t codec_bounds_bytes(size_t n) { return (size_t)bounds_grid(n) * sizeof(BoundsPartial); }

void codec_cube(const DeviceSoA &src, void *partial, CodecCube *cube, hipStream_t s) {
    const unsigned nb = src.npoints ? bounds_grid(src.npoints) : 0;
    if (nb) CW_LAUNCH("codec_bounds", codec_bounds_kernel, dim3(nb), dim3(CB), 0, s, src.x(), src.y(), src.z(), src.npoints, (BoundsPartial *)partial);
    CW_LAUNCH("codec_cube", codec_cube_kernel, dim3(1), dim3(64), 0, s, (const BoundsPartial *)partial, nb, cube);
}

bool codec_sort(const DeviceSoA &src, const CodecCube *cube, int bits, unsigned long long *keys, uint32_t *index, hipStream_t s) {
    const size_t n = src.npoints;
    if (!n) return true;
    CW_LAUNCH("codec_keys", codec_keys_kernel, dim3((unsigned)codec_blocks(n)), dim3(CB), 0, s, src.x(), src.y(), src.z(), n, cube, bits, keys, index);
    size_t tmp_bytes = 0;
    const unsigned end_bit = 3u * (unsigned)bits + 1u;
    hipError_t err = rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, keys + n, index, index + n, n, 0u, end_bit, s);
    void *tmp = nullptr;
    if (err == hipSuccess) {
        tmp = pool_alloc(tmp_bytes ? tmp_bytes : 256);
        if (!tmp) err = hipErrorOutOfMemory;
    }
    if (err == hipSuccess) {
        if (profiling_enabled()) profile_begin("radix_sort_pairs", s);
        err = rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys + n, index, index + n, n, 0u, end_bit, s);
        if (profiling_enabled()) profile_end(s);
    }
    tctx().free_later(tmp);
    if (err != hipSuccess) return hip_failed(err, "rocprim::radix_sort_pairs", __FILE__, __LINE__);
    return true;
}

void codec_count_scan(const unsigned long long *sorted_keys, size_t n, const CodecCube *cube, int bits, uint32_t *counts, unsigned long long *total_host,
                      uint32_t tag, hipStream_t s) {
    const size_t nb = codec_blocks(n);
    if (nb) CW_LAUNCH("codec_count", codec_count_kernel, dim3((unsigned)nb), dim3(CB), 0, s, sorted_keys, cube, bits, counts, nb);
    CW_LAUNCH("codec_scan", codec_scan_kernel, dim3((unsigned)bits), dim3(CB), 0, s, counts, nb, total_host, tag);
}

void codec_emit(const unsigned long long *sorted_keys, const uint32_t *sorted_index, const DeviceSoA &src, const CodecCube *cube, int sort_bits,
                const uint32_t *offsets, const CodecEmit &e, int colour_shift, hipStream_t s) {
    const size_t nb = codec_blocks(src.npoints);
    if (!nb || !e.nleaves) return;
    CW_LAUNCH("codec_emit", codec_emit_kernel, dim3((unsigned)nb), dim3(CB), 0, s, sorted_keys, sorted_index, src.rgbt(), cube, sort_bits, offsets, nb, e);
    CW_LAUNCH("codec_leaf", codec_leaf_kernel, dim3((unsigned)codec_blocks(e.nleaves)), dim3(CB), 0, s, e, colour_shift);
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(CB) codec_popcount_kernel(const uint8_t *__restrict__ occupancy, size_t n, uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_tot[CWAVES];
    const size_t i = (size_t)blockIdx.x * CB + threadIdx.x;
    const uint32_t v = block_sum<CB>(i < n ? (uint32_t)__popc((unsigned)occupancy[i]) : 0u, wave_tot);
    if (threadIdx.x == 0) counts[blockIdx.x] = v;
}

__global__ void __launch_bounds__(CB) codec_decode_scan_kernel(uint32_t *__restrict__ counts, size_t nblocks, unsigned long long *__restrict__ sink) {
    scan_block_counts<CB>(counts, nblocks, sink, 0u);
}

// node i of this depth -> its children, in child order, at offsets[workgroup] + the children of the workgroup's nodes before it
// (offsets == nullptr: one workgroup)
__global__ void __launch_bounds__(CB) codec_expand_kernel(const uint8_t *__restrict__ occupancy, const unsigned long long *__restrict__ prefix, size_t n,
                                                         const uint32_t *__restrict__ offsets, unsigned long long *__restrict__ out, size_t out_n) {
    __shared__ uint32_t wave_tot[CWAVES];
    const size_t i = (size_t)blockIdx.x * CB + threadIdx.x;
    const uint32_t byte = i < n ? occupancy[i] : 0u;
    const uint32_t c = (uint32_t)__popc(byte);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = c;
    for (int off = 1; off < 64; off <<= 1) {   // (kept: wave_inclusive_scan changed this kernel, and its times left the parent's spread)
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    size_t at = (offsets ? offsets[blockIdx.x] : 0u) + (inc - c);
    for (int w = 0; w < wave; w++) at += wave_tot[w];
    if (i >= n) return;
    const unsigned long long p = prefix[i] << 3;
    for (uint32_t child = 0; child < 8; child++) {
        if (!((byte >> child) & 1u)) continue;
        if (at < out_n) out[at] = p | child;
        at++;
    }
}

__global__ void __launch_bounds__(CB) codec_points_kernel(const unsigned long long *__restrict__ keys, CodecDecode d, float *__restrict__ ox, float *__restrict__ oy,
                                                         float *__restrict__ oz, uint32_t *__restrict__ ow) {
    const size_t j = (size_t)blockIdx.x * CB + threadIdx.x;
    if (j >= d.nleaves) return;
    uint32_t q[3];
    codec_unkey(keys[j], q);
    ox[j] = codec_position(d.mn[0], q[0], d.cell);
    oy[j] = codec_position(d.mn[1], q[1], d.cell);
    oz[j] = codec_position(d.mn[2], q[2], d.cell);
    const int cb = d.colour_bits, shift = 8 - cb;
    const uint64_t bit = (uint64_t)j * (uint64_t)(3 * cb);
    const uint64_t word = bit >> 5;
    const uint32_t off = (uint32_t)(bit & 31u);
    uint32_t packed = word < d.colour_words ? d.colours[word] >> off : 0u;
    if (off + 3u * (uint32_t)cb > 32u && word + 1 < d.colour_words) packed |= d.colours[word + 1] << (32u - off);
    const uint32_t mask = (1u << cb) - 1u;
    const uint32_t r = codec_colour_load(packed & mask, shift), g = codec_colour_load((packed >> cb) & mask, shift),
                   b = codec_colour_load((packed >> (2 * cb)) & mask, shift);
    const uint32_t tile = d.tiles ? d.tiles[j] : (uint32_t)d.tile_value;
    ow[j] = r | (g << 8) | (b << 16) | (tile << 24);
}

size_t codec_decode_scratch_words(const CodecDecode &d) {
    size_t most = 1;
    for (int depth = 1; depth < d.bits; depth++) most = most > d.nodes[depth - 1] ? most : d.nodes[depth - 1];
    return codec_blocks(most) + 4;   // the counts, their total, and an aligned 64-bit word the scan reports to
}

// occupancy: the device copy of the occupancy bytes; ping, pong: nleaves 64-bit words each; scratch: codec_decode_scratch_words()
unsigned long long *codec_expand(const uint8_t *occupancy, const CodecDecode &d, unsigned long long *ping, unsigned long long *pong, uint32_t *scratch,
                                 hipStream_t s) {
    (void)hipMemsetAsync(ping, 0, sizeof(unsigned long long), s);   // the root: the empty prefix
    size_t at = 0;
    for (int depth = 0; depth < d.bits; depth++) {
        const size_t n = depth == 0 ? 1 : d.nodes[depth - 1], out_n = d.nodes[depth];
        const size_t nb = codec_blocks(n);
        const uint32_t *offsets = nullptr;
        if (nb > 1) {
            CW_LAUNCH("codec_popcount", codec_popcount_kernel, dim3((unsigned)nb), dim3(CB), 0, s, occupancy + at, n, scratch);
            CW_LAUNCH("codec_decode_scan", codec_decode_scan_kernel, dim3(1), dim3(CB), 0, s, scratch, nb, (unsigned long long *)(scratch + ((nb + 2) & ~(size_t)1)));
            offsets = scratch;
        }
        CW_LAUNCH("codec_expand", codec_expand_kernel, dim3((unsigned)nb), dim3(CB), 0, s, occupancy + at, ping, n, offsets, pong, out_n);
        at += n;
        unsigned long long *t = ping; ping = pong; pong = t;
    }
    return ping;
}

void codec_decode(const uint8_t *occupancy, const CodecDecode &d, unsigned long long *ping, unsigned long long *pong, uint32_t *scratch, const DeviceSoA &dst,
                  hipStream_t s) {
    if (!d.nleaves) return;
    ping = codec_expand(occupancy, d, ping, pong, scratch, s);
    CW_LAUNCH("codec_points", codec_points_kernel, dim3((unsigned)codec_blocks(d.nleaves)), dim3(CB), 0, s, ping, d, dst.x(), dst.y(), dst.z(), dst.rgbt());
}

}  // namespace k
}  // namespace cwipc_amd
