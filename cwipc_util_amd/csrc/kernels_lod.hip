// kernels_lod.hip -- gfx950 kernels of level-of-detail decoding (RULE L: hip_ext.h; the arithmetic: lod_terms.hpp).
//
// A decoder that hands out at most t of a packet's b octree bits makes the cloud of L(P, t) without making the packet.  A new leaf is
// a node of depth t; its members are the leaves beneath it, a contiguous run in key order.
//
// Runs.  From a packet body: first[] (transform_prepare's one scan over all occupancy bytes) names every node's first child, so the
// run of node j of depth t starts b - t dependent lookups below it and ends where the next node's starts: one lane per new leaf, no
// key or point of the depths below t is made.  From a frame's leaves (RULE P keeps them with their full keys): a leaf starts a run
// where its prefix of t triples differs from its predecessor's; count, scan, scatter give the starts and the new keys, and their
// number is the one word the host waits for (a delta packet's header does not hold the node counts of its frame).
//
// Reduction.  One lane per OLD leaf, whatever the run lengths (1 .. nleaves): a workgroup's first lane searches the starts for its
// run, the others search only the at most 256 runs behind it (a run holds a leaf at least), the number goes through LDS.  A
// segmented scan over the wave adds the three stored values and ORs the tiles within a run; the last lane of a run in a wave stores
// the sums when the whole run lies in the wave and adds them with integer atomics when it crosses a wave's boundary.  Integer sums
// are order-free, so the bytes do not depend on the schedule.  A wave's share of a channel is at most 64 x 255; the sums are 64 bits.
//
// Points.  One lane per new leaf: the centre of its cell at depth t, the rounded means, the tile.
// Every load is bounded by the counts the launcher was given and every store by the new leaf count, whatever the bytes.
#include "internal.hpp"
#include "block_scan.hpp"
#include "lod_terms.hpp"

namespace cwipc_amd {
namespace k {

static constexpr int LB = 256;   // lanes per workgroup, one leaf each
static constexpr int LWAVES = LB / 64;

static unsigned lod_blocks(size_t n) { return (unsigned)((n + LB - 1) / LB); }

// ---------------------------------------------------------------------------
// runs
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(LB) lod_tree_runs_kernel(const uint32_t *__restrict__ first, uint32_t inner, uint32_t begin, int steps, uint32_t nruns,
                                                          uint32_t nleaves, uint32_t *__restrict__ start) {
    const size_t j = (size_t)blockIdx.x * LB + threadIdx.x;
    if (j > nruns) return;
    uint32_t leaf = nleaves;
    if (j < nruns) {
        uint64_t g = (uint64_t)begin + j;
        for (int s = 0; s < steps; s++) g = g < inner ? first[g] : (uint64_t)inner + nleaves;
        leaf = g >= inner && g - inner < nleaves ? (uint32_t)(g - inner) : nleaves;
    }
    start[j] = leaf;
}

__device__ __forceinline__ bool lod_head_at(const unsigned long long *__restrict__ keys, size_t i, size_t n, int b, int t) {
    return i < n && lod_run_head(i ? keys[i - 1] : 0ull, keys[i], b, t, i == 0);
}

__global__ void __launch_bounds__(LB) lod_heads_count_kernel(const unsigned long long *__restrict__ keys, size_t n, int b, int t, uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_lds[LWAVES];
    const size_t i = (size_t)blockIdx.x * LB + threadIdx.x;
    const uint32_t v = block_sum<LB>(lod_head_at(keys, i, n, b, t) ? 1u : 0u, wave_lds);
    if (threadIdx.x == 0) counts[blockIdx.x] = v;
}

__global__ void __launch_bounds__(LB) lod_heads_scan_kernel(uint32_t *__restrict__ counts, size_t nblocks, unsigned long long *__restrict__ total_host, uint32_t tag) {
    scan_block_counts<LB>(counts, nblocks, total_host, tag);
}

// run r starts at leaf start[r] and has the key cut[r]; start[the number of runs] = n
__global__ void __launch_bounds__(LB) lod_heads_scatter_kernel(const unsigned long long *__restrict__ keys, size_t n, int b, int t, const uint32_t *__restrict__ offsets,
                                                              uint32_t *__restrict__ start, unsigned long long *__restrict__ cut) {
    __shared__ uint32_t wave_lds[LWAVES];
    const size_t i = (size_t)blockIdx.x * LB + threadIdx.x;
    const bool head = lod_head_at(keys, i, n, b, t);
    const uint32_t rank = offsets[blockIdx.x] + block_exclusive_scan<LB>(head ? 1u : 0u, wave_lds, nullptr);
    if (i >= n) return;
    if (head && rank < n) {
        start[rank] = (uint32_t)i;
        cut[rank] = lod_prefix(keys[i], b, t);
    }
    if (i == n - 1 && rank + (head ? 1u : 0u) <= n) start[rank + (head ? 1u : 0u)] = (uint32_t)n;
}

// ---------------------------------------------------------------------------
// reduction
// ---------------------------------------------------------------------------
// the largest r in [lo, hi) with start[r] <= i, given start[lo] <= i < start[hi]
__device__ __forceinline__ uint32_t lod_run_of(const uint32_t *__restrict__ start, uint32_t lo, uint32_t hi, uint32_t i) {
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (start[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(LB) lod_reduce_kernel(LodSource src, const uint32_t *__restrict__ start, uint32_t nruns, CodecLeafSum *__restrict__ sums) {
    __shared__ uint32_t first_run;
    const size_t i = (size_t)blockIdx.x * LB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < (size_t)src.nleaves;
    if (threadIdx.x == 0) first_run = lod_run_of(start, 0u, nruns, (uint32_t)i);   // (the grid has no workgroup without a leaf)
    __syncthreads();
    uint32_t run = 0xffffffffu, r = 0, g = 0, b = 0, tile = 0;
    if (valid) {
        const uint32_t lo = first_run;
        const uint64_t most = (uint64_t)lo + threadIdx.x + 1u;   // a run holds a leaf at least: leaf i lies in front of run lo + its lane + 1
        run = lod_run_of(start, lo, most < nruns ? (uint32_t)most : nruns, (uint32_t)i);
        if (src.packed) {
            const int cb = src.colour_bits;
            const uint64_t bit = (uint64_t)i * (uint64_t)(3 * cb);
            const uint64_t word = bit >> 5;
            const uint32_t off = (uint32_t)(bit & 31u);
            uint32_t packed = word < src.colour_words ? src.packed[word] >> off : 0u;
            if (off + 3u * (uint32_t)cb > 32u && word + 1 < src.colour_words) packed |= src.packed[word + 1] << (32u - off);
            const uint32_t mask = (1u << cb) - 1u;
            r = packed & mask;
            g = (packed >> cb) & mask;
            b = (packed >> (2 * cb)) & mask;
        } else {
            r = src.planes[i];
            g = src.planes[(size_t)src.nleaves + i];
            b = src.planes[2 * (size_t)src.nleaves + i];
        }
        tile = src.tiles ? (uint32_t)src.tiles[i] : (uint32_t)src.tile_value;
    }
    for (int off = 1; off < 64; off <<= 1) {   // (a segmented scan: four values a step, folded only within a run)
        const uint32_t o_run = __shfl_up(run, off, 64), o_r = __shfl_up(r, off, 64), o_g = __shfl_up(g, off, 64), o_b = __shfl_up(b, off, 64),
                       o_tile = __shfl_up(tile, off, 64);
        if (lane >= off && o_run == run) { r += o_r; g += o_g; b += o_b; tile |= o_tile; }
    }
    const uint32_t next_run = __shfl_down(run, 1, 64);
    if (!valid || run >= nruns || !(lane == 63 || next_run != run)) return;
    CodecLeafSum *s = sums + run;
    const size_t wave_first = i - (size_t)lane;
    if ((size_t)start[run] >= wave_first && (size_t)start[run + 1] == i + 1) {   // the whole run lies in this wave: nobody else writes its sums
        s->r = r;
        s->g = g;
        s->b = b;
        s->tile = tile;
    } else {
        atomicAdd(&s->r, (unsigned long long)r);
        atomicAdd(&s->g, (unsigned long long)g);
        atomicAdd(&s->b, (unsigned long long)b);
        atomicOr(&s->tile, tile);
    }
}

// ---------------------------------------------------------------------------
// points
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(LB) lod_points_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ start,
                                                       const CodecLeafSum *__restrict__ sums, CodecDecode d, float *__restrict__ ox, float *__restrict__ oy,
                                                       float *__restrict__ oz, uint32_t *__restrict__ ow) {
    const size_t j = (size_t)blockIdx.x * LB + threadIdx.x;
    if (j >= d.nleaves) return;
    uint32_t q[3];
    codec_unkey(keys[j], q);
    ox[j] = codec_position(d.mn[0], q[0], d.cell);
    oy[j] = codec_position(d.mn[1], q[1], d.cell);
    oz[j] = codec_position(d.mn[2], q[2], d.cell);
    const uint32_t a = start[j], e = start[j + 1], n = e > a ? e - a : 1u;
    const CodecLeafSum s = sums[j];
    const int shift = 8 - d.colour_bits;
    const uint32_t r = codec_colour_load(lod_mean(s.r, n), shift), g = codec_colour_load(lod_mean(s.g, n), shift), b = codec_colour_load(lod_mean(s.b, n), shift);
    ow[j] = r | (g << 8) | (b << 16) | ((s.tile & 255u) << 24);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void lod_runs_of_tree(const uint32_t *first, uint32_t inner, uint32_t begin, int steps, uint32_t nruns, uint32_t nleaves, uint32_t *start, hipStream_t s) {
    CW_LAUNCH("lod_tree_runs", lod_tree_runs_kernel, dim3(lod_blocks((size_t)nruns + 1)), dim3(LB), 0, s, first, inner, begin, steps, nruns, nleaves, start);
}

size_t lod_key_runs_words(size_t n) { return (size_t)lod_blocks(n) + 4; }

void lod_runs_of_keys(const unsigned long long *keys, uint32_t n, int b, int t, uint32_t *start, unsigned long long *cut, uint32_t *counts,
                      unsigned long long *total_host, uint32_t tag, hipStream_t s) {
    const unsigned nb = lod_blocks(n);
    if (!nb) return;
    CW_LAUNCH("lod_heads_count", lod_heads_count_kernel, dim3(nb), dim3(LB), 0, s, keys, (size_t)n, b, t, counts);
    CW_LAUNCH("lod_heads_scan", lod_heads_scan_kernel, dim3(1), dim3(LB), 0, s, counts, (size_t)nb, total_host, tag);
    CW_LAUNCH("lod_heads_scatter", lod_heads_scatter_kernel, dim3(nb), dim3(LB), 0, s, keys, (size_t)n, b, t, counts, start, cut);
}

bool lod_points(const LodSource &src, const uint32_t *start, uint32_t nruns, const unsigned long long *cut, CodecLeafSum *sums, const CodecDecode &d,
                const DeviceSoA &dst, hipStream_t s) {
    if (!src.nleaves || !nruns || d.nleaves != nruns) return true;
    if (hipMemsetAsync(sums, 0, (size_t)nruns * sizeof(CodecLeafSum), s) != hipSuccess) return false;
    CW_LAUNCH("lod_reduce", lod_reduce_kernel, dim3(lod_blocks(src.nleaves)), dim3(LB), 0, s, src, start, nruns, sums);
    CW_LAUNCH("lod_points", lod_points_kernel, dim3(lod_blocks(nruns)), dim3(LB), 0, s, cut, start, (const CodecLeafSum *)sums, d, dst.x(), dst.y(), dst.z(), dst.rgbt());
    return true;
}

}  // namespace k
}  // namespace cwipc_amd
