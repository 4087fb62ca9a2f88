// kernels_floor.hip -- gfx950 kernels of the registration pipeline's floor and tile helpers
// (reference python/cwipc/registration/util.py:146-229): the stable two-class partition behind cwipc_floor_filter,
// cwipc_randomize_floor and cwipc_limit_floor_to_radius, the seeded tile shuffle, the two order statistics
// cwipc_compute_radius interpolates between, the tile histogram of cwipc_compute_tile_occupancy and the bounds of the
// analyze filter.  All of them stream the SoA planes once per pass, 16 bytes per lane and plane; none of them is a
// mode of the timed tile / crop compaction in kernels_basic.hip.
//
// A point is FLOOR iff (double)y < level -- numpy's `column < scalar` on a float32 column, the scalar's conversion being
// the caller's (util.py: _threshold); a NaN y is therefore not floor.
#include "internal.hpp"
#include "counter_rng.hpp"
#include "plane_seg_terms.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>

namespace cwipc_amd {
namespace k {

static constexpr int FBLOCK = 256;
static constexpr int FWAVES = FBLOCK / 64;
static constexpr int FITEMS = 4;                      // points per lane: one dwordx4 per plane
static constexpr int FTILE = FBLOCK * FITEMS;         // 1024 points per workgroup

size_t floor_blocks(size_t n) { return (n + FTILE - 1) / FTILE; }

static inline unsigned stream_grid(size_t n) {
    size_t g = (n + FTILE - 1) / FTILE;
    if (g < 1) g = 1;
    if (g > 512) g = 512;   // grid-stride beyond two workgroups per CU: a workgroup's histogram flush then stands against 4 k points and more
    return (unsigned)g;
}

// numpy.linalg.norm(..., axis=1) of float32 rows: the squares, added up in index order, every operation rounded to
// float32 on its own (the build passes -ffp-contract=off; the intrinsics say so again)
__device__ __forceinline__ float sum_squares(float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
}
// ... and its root: the f64 root of a float32, rounded to float32, is the correctly rounded float32 root
__device__ __forceinline__ float root_f32(float s) { return (float)sqrt((double)s); }

// The lane's FITEMS consecutive values of one plane from `base` on; values beyond n read as `pad`.
template <typename T4, typename T>
__device__ __forceinline__ void load_items(const T *__restrict__ plane, size_t base, size_t n, T pad, T (&v)[FITEMS]) {
    if (base + FITEMS <= n) {
        const T4 q = *reinterpret_cast<const T4 *>(plane + base);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < FITEMS; j++) v[j] = base + j < n ? plane[base + j] : pad;
    }
}

// ---------------------------------------------------------------------------
// a. stable two-class partition
// ---------------------------------------------------------------------------
// Class A (first in the output) and class B (behind it) of the lane's points as two 4-bit masks.
__device__ __forceinline__ void classify(const FloorArgs &a, const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                         size_t base, size_t n, unsigned &ma, unsigned &mb) {
    ma = mb = 0;
    if (base >= n) return;
    float vy[FITEMS];
    load_items<float4>(y, base, n, 0.f, vy);
    float vx[FITEMS] = {0, 0, 0, 0}, vz[FITEMS] = {0, 0, 0, 0};
    const bool limit = (a.flags & FLOOR_LIMIT_RADIUS) != 0;
    if (limit) {
        load_items<float4>(x, base, n, 0.f, vx);
        load_items<float4>(z, base, n, 0.f, vz);
    }
    const bool keep_floor = (a.flags & (FLOOR_KEEP_FLOOR | FLOOR_LIMIT_RADIUS)) != 0, keep_rest = (a.flags & FLOOR_KEEP_REST) != 0;
#pragma unroll
    for (int j = 0; j < FITEMS; j++) {
        if (base + j >= n) break;
        const bool is_floor = (double)vy[j] < a.level;
        bool first = keep_floor && is_floor;
        if (first && limit) first = (double)root_f32(sum_squares(vx[j], vy[j], vz[j])) < a.radius;
        if (first) ma |= 1u << j;
        if (keep_rest && !is_floor) mb |= 1u << j;
    }
}

// The same two masks under RULE S (hip_ext.h): class A the inliers of a plane -- with PLANE_BELOW_IS_INLIER everything with
// e <= distance --, class B the other points; a non-finite point gives a NaN or an infinity and is not an inlier.
__device__ __forceinline__ void classify(const PlaneArgs &a, const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                         size_t base, size_t n, unsigned &ma, unsigned &mb) {
    ma = mb = 0;
    if (base >= n) return;
    float vx[FITEMS], vy[FITEMS], vz[FITEMS];
    load_items<float4>(x, base, n, 0.f, vx);
    load_items<float4>(y, base, n, 0.f, vy);
    load_items<float4>(z, base, n, 0.f, vz);
    const bool keep_in = (a.flags & CWIPC_HIP_PLANE_KEEP_INLIERS) != 0, keep_rest = (a.flags & CWIPC_HIP_PLANE_KEEP_REST) != 0;
    const bool below = (a.flags & CWIPC_HIP_PLANE_BELOW_IS_INLIER) != 0;
#pragma unroll
    for (int j = 0; j < FITEMS; j++) {
        if (base + j >= n) break;
        const double e = plane_e(a.plane, (double)vx[j], (double)vy[j], (double)vz[j]);
        const bool in = below ? plane_below(e, a.distance) : plane_inlier(e, a.distance);
        if (keep_in && in) ma |= 1u << j;
        if (keep_rest && !in) mb |= 1u << j;
    }
}

// Points of the wave's lanes in front of this lane, and in the whole wave, that a mask selects: one ballot and one
// popcount per item (the points run lane-major, a lane's four in a row).
__device__ __forceinline__ void wave_rank(unsigned m, uint32_t &before, uint32_t &total) {
    const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
    before = total = 0;
#pragma unroll
    for (int j = 0; j < FITEMS; j++) {
        const unsigned long long b = __ballot((m >> j) & 1u);
        before += (uint32_t)__popcll(b & below);
        total += (uint32_t)__popcll(b);
    }
}

// counts[b] = class A points of workgroup b's tile, counts[gridDim.x + b] = class B points
template <class Args>
__global__ void __launch_bounds__(FBLOCK) floor_count_kernel(Args a, const float *__restrict__ x, const float *__restrict__ y,
                                                            const float *__restrict__ z, size_t n, uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_tot[2][FWAVES];
    const size_t base = (size_t)blockIdx.x * FTILE + (size_t)threadIdx.x * FITEMS;
    unsigned ma, mb;
    classify(a, x, y, z, base, n, ma, mb);
    uint32_t before, ta, tb;
    wave_rank(ma, before, ta);
    wave_rank(mb, before, tb);
    if ((threadIdx.x & 63) == 0) { wave_tot[0][threadIdx.x >> 6] = ta; wave_tot[1][threadIdx.x >> 6] = tb; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t t = 0;
        for (int w = 0; w < FWAVES; w++) t += wave_tot[threadIdx.x][w];
        counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

// One workgroup: counts[0, nb) and counts[nb, 2 nb) become exclusive prefix sums (each from 0), counts[2 nb] and
// counts[2 nb + 1] the two totals, which also go to two pinned 64-bit host words with `tag` in their upper halves.
static constexpr int FSCAN = 256;   // (2 M points are 2 k counts per class: eight rounds)
__global__ void __launch_bounds__(FSCAN) floor_scan_kernel(uint32_t *__restrict__ counts, size_t nb, unsigned long long *__restrict__ total_host, uint32_t tag) {
    __shared__ uint32_t wave_tot[FSCAN / 64];
    __shared__ uint32_t carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int cls = 0; cls < 2; cls++) {
        uint32_t *cnt = counts + (size_t)cls * nb;
        if (threadIdx.x == 0) carry = 0;
        __syncthreads();
        for (size_t base = 0; base < nb; base += FSCAN) {
            const size_t i = base + threadIdx.x;
            const uint32_t v = i < nb ? cnt[i] : 0;
            uint32_t inc = v;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t t = __shfl_up(inc, off, 64);
                if (lane >= off) inc += t;
            }
            if (lane == 63) wave_tot[wave] = inc;
            __syncthreads();
            uint32_t wave_base = 0;
            for (int w = 0; w < wave; w++) wave_base += wave_tot[w];
            const uint32_t c = carry;
            if (i < nb) cnt[i] = c + wave_base + inc - v;
            __syncthreads();
            if (threadIdx.x == FSCAN - 1) carry = c + wave_base + inc;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            counts[2 * nb + cls] = carry;
            __hip_atomic_store(total_host + cls, ((unsigned long long)tag << 32) | carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
    }
}

// Every class A point to offsets[b] + its rank in the tile, every class B point to total A + offsets[nb + b] + its rank.
template <class Args>
__global__ void __launch_bounds__(FBLOCK) floor_scatter_kernel(Args a, const float *__restrict__ x, const float *__restrict__ y,
                                                              const float *__restrict__ z, const uint32_t *__restrict__ rgbt, size_t n,
                                                              const uint32_t *__restrict__ offsets, float *__restrict__ ox, float *__restrict__ oy,
                                                              float *__restrict__ oz, uint32_t *__restrict__ ow, size_t out_n) {
    __shared__ uint32_t wave_tot[2][FWAVES];
    const size_t base = (size_t)blockIdx.x * FTILE + (size_t)threadIdx.x * FITEMS;
    unsigned ma, mb;
    classify(a, x, y, z, base, n, ma, mb);
    uint32_t ra, ta, rb, tb;
    wave_rank(ma, ra, ta);
    wave_rank(mb, rb, tb);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wave_tot[0][wave] = ta; wave_tot[1][wave] = tb; }
    __syncthreads();
    for (int w = 0; w < wave; w++) { ra += wave_tot[0][w]; rb += wave_tot[1][w]; }
    if (!(ma | mb)) return;
    const size_t nb = gridDim.x;
    size_t at_a = (size_t)offsets[blockIdx.x] + ra;
    size_t at_b = (size_t)offsets[2 * nb] + offsets[nb + blockIdx.x] + rb;
    float vx[FITEMS], vy[FITEMS], vz[FITEMS];
    uint32_t vw[FITEMS];
    load_items<float4>(x, base, n, 0.f, vx);
    load_items<float4>(y, base, n, 0.f, vy);
    load_items<float4>(z, base, n, 0.f, vz);
    load_items<uint4>(rgbt, base, n, 0u, vw);
#pragma unroll
    for (int j = 0; j < FITEMS; j++) {
        const bool fa = (ma >> j) & 1u, fb = (mb >> j) & 1u;
        if (!(fa || fb)) continue;
        const size_t o = fa ? at_a++ : at_b++;
        if (o >= out_n) continue;   // (cannot happen: the counts come from the same predicate)
        ox[o] = vx[j]; oy[o] = vy[j]; oz[o] = vz[j]; ow[o] = vw[j];
    }
}

template <class Args>
static void partition_count(const char *name, const DeviceSoA &src, const Args &a, uint32_t *counts, hipStream_t s) {
    const size_t nb = floor_blocks(src.npoints);
    if (!nb) return;
    CW_LAUNCH(name, floor_count_kernel<Args>, dim3((unsigned)nb), dim3(FBLOCK), 0, s, a, src.x(), src.y(), src.z(), src.npoints, counts);
}

void floor_scan(uint32_t *counts, size_t nb, unsigned long long *total_host, uint32_t tag, hipStream_t s) {
    CW_LAUNCH("floor_scan", floor_scan_kernel, dim3(1), dim3(FSCAN), 0, s, counts, nb, total_host, tag);
}

template <class Args>
static void partition_scatter(const char *name, const DeviceSoA &src, const Args &a, const uint32_t *offsets, const DeviceSoA &dst, hipStream_t s) {
    const size_t nb = floor_blocks(src.npoints);
    if (!nb || !dst.npoints) return;
    CW_LAUNCH(name, floor_scatter_kernel<Args>, dim3((unsigned)nb), dim3(FBLOCK), 0, s, a, src.x(), src.y(), src.z(), src.rgbt(), src.npoints, offsets,
              dst.x(), dst.y(), dst.z(), dst.rgbt(), dst.npoints);
}

void floor_count(const DeviceSoA &src, const FloorArgs &a, uint32_t *counts, hipStream_t s) { partition_count("floor_count", src, a, counts, s); }
void floor_count(const DeviceSoA &src, const PlaneArgs &a, uint32_t *counts, hipStream_t s) { partition_count("plane_count", src, a, counts, s); }
void floor_scatter(const DeviceSoA &src, const FloorArgs &a, const uint32_t *offsets, const DeviceSoA &dst, hipStream_t s) {
    partition_scatter("floor_scatter", src, a, offsets, dst, s);
}
void floor_scatter(const DeviceSoA &src, const PlaneArgs &a, const uint32_t *offsets, const DeviceSoA &dst, hipStream_t s) {
    partition_scatter("plane_scatter", src, a, offsets, dst, s);
}

// ---------------------------------------------------------------------------
// b. tile shuffle within the first n_first points
// ---------------------------------------------------------------------------
// (splitmix64: counter_rng.hpp)
__global__ void __launch_bounds__(FBLOCK) shuffle_keys_kernel(unsigned long long seed, size_t n_first, unsigned long long *__restrict__ keys,
                                                             uint32_t *__restrict__ index) {
    for (size_t i = (size_t)blockIdx.x * FBLOCK + threadIdx.x; i < n_first; i += (size_t)gridDim.x * FBLOCK) {
        keys[i] = splitmix64(seed + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull);
        index[i] = (uint32_t)i;
    }
}

// position j < n_first keeps its colour and takes the tile byte of point perm[j]; the words behind are copied
__global__ void __launch_bounds__(FBLOCK) shuffle_apply_kernel(const uint32_t *__restrict__ rgbt, const uint32_t *__restrict__ perm, size_t n_first, size_t n,
                                                              uint32_t *__restrict__ ow) {
    for (size_t i = (size_t)blockIdx.x * FBLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * FBLOCK) {
        uint32_t w = rgbt[i];
        if (i < n_first) {
            const uint32_t from = perm[i];
            if (from < n_first) w = (w & 0x00ffffffu) | (rgbt[from] & 0xff000000u);
        }
        ow[i] = w;
    }
}

bool floor_shuffle(const uint32_t *rgbt, size_t n_first, size_t n, uint64_t seed, uint32_t *out_rgbt, hipStream_t s) {
    if (!n) return true;
    // one block: keys in | keys out | index in | index out (the stable ascending sort of the keys is the permutation)
    unsigned long long *keys = nullptr;
    uint32_t *index = nullptr;
    void *sort_tmp = nullptr;
    bool ok = true;
    if (n_first > 1) {
        keys = (unsigned long long *)pool_alloc(n_first * 8 * 2);
        index = (uint32_t *)pool_alloc(n_first * 4 * 2);
        ok = keys && index;
        if (ok) {
            CW_LAUNCH("floor_shuffle_keys", shuffle_keys_kernel, dim3(stream_grid(n_first)), dim3(FBLOCK), 0, s, (unsigned long long)seed, n_first, keys, index);
            size_t tmp_bytes = 0;
            hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, keys + n_first, index, index + n_first, n_first, 0u, 64u, s);
            if (e == hipSuccess) {
                sort_tmp = pool_alloc(tmp_bytes ? tmp_bytes : 256);
                if (!sort_tmp) e = hipErrorOutOfMemory;
            }
            if (e == hipSuccess) {
                if (profiling_enabled()) profile_begin("radix_sort_pairs", s);
                e = rocprim::radix_sort_pairs(sort_tmp, tmp_bytes, keys, keys + n_first, index, index + n_first, n_first, 0u, 64u, s);
                if (profiling_enabled()) profile_end(s);
            }
            if (e != hipSuccess) ok = hip_failed(e, "rocprim::radix_sort_pairs", __FILE__, __LINE__);
        }
    }
    if (ok) {
        // (no floor to speak of: n_first = 0 for the kernel, a plain copy of the words)
        CW_LAUNCH("floor_shuffle_apply", shuffle_apply_kernel, dim3(stream_grid(n)), dim3(FBLOCK), 0, s, rgbt, index ? index + n_first : nullptr,
                  index ? n_first : (size_t)0, n, out_rgbt);
    }
    // the blocks go back to the pool when the stream has been waited for (the caller's sync)
    ThreadCtx &c = tctx();
    c.free_later(keys);
    c.free_later(index);
    c.free_later(sort_tmp);
    return ok;
}

// ---------------------------------------------------------------------------
// c. order statistics of the distance from the y axis, per class
// ---------------------------------------------------------------------------
// Exact selection by four radix passes (8 bits each, from the top) over the bit pattern of s = (x*x + 0) + z*z, a
// non-negative float32 whose order is the order of its bits (NaN counts as the largest value, as numpy.sort has it); the
// root is monotone, so the roots of the two winners are the two order statistics of d = sqrt(s).  Four selectors: class
// (0 floor, 1 rest) x (rank lo, rank lo + 1).  State, 32-bit words in device memory, zeroed by the caller:
//   [0, 2) the class counts   [2, 6) the four statistics (float bits)   [8, 12) prefix per selector   [12, 16) rank per selector
//   [16, 20) 1: the selector has its own histogram this pass (0: the class's lo selector has the same prefix)
//   [32, 32 + 4 * 4 * 256) histograms per pass and selector
static constexpr int SEL_PREFIX = 8, SEL_RANK = 12, SEL_OWN = 16, SEL_HIST = 32;

__device__ __forceinline__ uint32_t distance_key(float x, float z) {
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(x, x), 0.f), __fmul_rn(z, z));
    return s != s ? 0x7fc00000u : __float_as_uint(s);
}

__global__ void __launch_bounds__(FBLOCK) radius_hist_kernel(int pass, double level, const float *__restrict__ x, const float *__restrict__ y,
                                                            const float *__restrict__ z, size_t n, uint32_t *__restrict__ state) {
    __shared__ uint32_t hist[4][256];
    for (int i = threadIdx.x; i < 4 * 256; i += FBLOCK) (&hist[0][0])[i] = 0;
    __shared__ uint32_t prefix[4], own[4];
    if (threadIdx.x < 4) { prefix[threadIdx.x] = state[SEL_PREFIX + threadIdx.x]; own[threadIdx.x] = state[SEL_OWN + threadIdx.x]; }
    __syncthreads();
    const int shift = 24 - 8 * pass;           // the digit of this pass
    for (size_t tile = blockIdx.x; tile * FTILE < n; tile += gridDim.x) {
        const size_t base = tile * FTILE + (size_t)threadIdx.x * FITEMS;
        if (base >= n) continue;
        float vx[FITEMS], vy[FITEMS], vz[FITEMS];
        load_items<float4>(x, base, n, 0.f, vx);
        load_items<float4>(y, base, n, 0.f, vy);
        load_items<float4>(z, base, n, 0.f, vz);
#pragma unroll
        for (int j = 0; j < FITEMS; j++) {
            if (base + j >= n) break;
            const int cls = (double)vy[j] < level ? 0 : 1;
            const uint32_t key = distance_key(vx[j], vz[j]);
            const uint32_t digit = (key >> shift) & 255u;
            const uint32_t high = pass == 0 ? 0u : key >> (shift + 8);
            if (high == prefix[2 * cls]) atomicAdd(&hist[2 * cls][digit], 1u);
            if (own[2 * cls + 1] && high == prefix[2 * cls + 1]) atomicAdd(&hist[2 * cls + 1][digit], 1u);
        }
    }
    __syncthreads();
    uint32_t *out = state + SEL_HIST + (size_t)pass * 4 * 256;
    for (int i = threadIdx.x; i < 4 * 256; i += FBLOCK) {
        const uint32_t v = (&hist[0][0])[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// One wave, lane s < 4 for selector s: the bin of this pass's histogram that holds the selector's rank.  After the first pass
// the class counts are known and with them the ranks: lo = floor((n - 1) * 0.99) with the product in float32 -- numpy.percentile
// divides 99 by float32(100) for float32 data and multiplies in that type -- and min(lo + 1, n - 1).  After the last pass
// the prefix is the whole key.
__global__ void __launch_bounds__(64) radius_pick_kernel(int pass, uint32_t *__restrict__ state) {
    const int s = threadIdx.x;
    if (s >= 4) return;
    const int cls = s >> 1;
    const uint32_t *hist = state + SEL_HIST + (size_t)pass * 4 * 256 + (size_t)(state[SEL_OWN + s] ? s : 2 * cls) * 256;
    uint32_t rank = state[SEL_RANK + s];
    uint32_t count = state[cls];
    if (pass == 0) {
        count = 0;
        for (int b = 0; b < 256; b++) count += hist[b];
        uint32_t lo = 0;
        if (count) {
            lo = (uint32_t)floorf(__fmul_rn((float)(count - 1), 0.99f));
            if (lo > count - 1) lo = count - 1;
        }
        rank = (s & 1) ? (count && lo + 1 <= count - 1 ? lo + 1 : lo) : lo;
    }
    uint32_t bin = 0, before = 0;
    if (count) {
        for (; bin < 255; bin++) {
            const uint32_t h = hist[bin];
            if (rank < before + h) break;
            before += h;
        }
    }
    const uint32_t prefix = (pass == 0 ? 0u : state[SEL_PREFIX + s] << 8) | bin;
    rank -= before;
    // every lane has read what it needs of the shared words before any of them is written
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t lo_prefix = __shfl(prefix, 2 * cls, 64);
    state[SEL_PREFIX + s] = prefix;
    state[SEL_RANK + s] = rank;
    state[SEL_OWN + s] = (s & 1) && prefix != lo_prefix ? 1u : 0u;
    if (pass == 0 && !(s & 1)) state[cls] = count;
    if (pass == 3) state[2 + s] = count ? __float_as_uint(root_f32(__uint_as_float(prefix))) : 0x7fc00000u;
}

size_t floor_radius_state_bytes() { return (size_t)(SEL_HIST + 4 * 4 * 256) * sizeof(uint32_t); }

void floor_radius_select(const DeviceSoA &src, double level, uint32_t *state, hipStream_t s) {
    (void)hipMemsetAsync(state, 0, floor_radius_state_bytes(), s);
    for (int pass = 0; pass < 4; pass++) {
        if (src.npoints)
            CW_LAUNCH("floor_radius_hist", radius_hist_kernel, dim3(stream_grid(src.npoints)), dim3(FBLOCK), 0, s, pass, level, src.x(), src.y(), src.z(),
                      src.npoints, state);
        CW_LAUNCH("floor_radius_pick", radius_pick_kernel, dim3(1), dim3(64), 0, s, pass, state);
    }
}

// ---------------------------------------------------------------------------
// d. tile histogram
// ---------------------------------------------------------------------------
// A histogram per wave in LDS: a cloud has a handful of tile values, and a wave whose lanes all hold the same one (the usual
// case: a camera's points lie together) adds its count with one atomic instead of 64 on one address.
__global__ void __launch_bounds__(FBLOCK) tile_hist_kernel(int nonfloor_only, double level, const float *__restrict__ y, const uint32_t *__restrict__ rgbt, size_t n,
                                                          unsigned long long *__restrict__ counts) {
    __shared__ uint32_t hist[FWAVES][256];
    for (int i = threadIdx.x; i < FWAVES * 256; i += FBLOCK) (&hist[0][0])[i] = 0;
    __syncthreads();
    uint32_t *mine = hist[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    // (a workgroup sees n / gridDim.x + FTILE points at most: 32 bits do until the flush)
    for (size_t tile = blockIdx.x; tile * FTILE < n; tile += gridDim.x) {   // (the trip count is the same for all lanes of a wave)
        const size_t base = tile * FTILE + (size_t)threadIdx.x * FITEMS;
        uint32_t vw[FITEMS] = {0, 0, 0, 0};
        float vy[FITEMS] = {0, 0, 0, 0};
        if (base < n) {
            load_items<uint4>(rgbt, base, n, 0u, vw);
            if (nonfloor_only) load_items<float4>(y, base, n, 0.f, vy);
        }
#pragma unroll
        for (int j = 0; j < FITEMS; j++) {
            const bool counted = base + j < n && !(nonfloor_only && (double)vy[j] < level);
            const uint32_t t = vw[j] >> 24;
            const unsigned long long who = __ballot(counted);
            if (!who) continue;
            const uint32_t t0 = (uint32_t)__shfl((int)t, __builtin_ctzll(who), 64);
            if (__ballot(counted && t != t0) == 0ull) {
                if (lane == 0) atomicAdd(&mine[t0], (uint32_t)__popcll(who));
            } else if (counted) {
                atomicAdd(&mine[t], 1u);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 256; t += FBLOCK) {
        unsigned long long v = 0;
        for (int w = 0; w < FWAVES; w++) v += hist[w][t];
        if (v) atomicAdd(&counts[t], v);
    }
}

void tile_histogram(const DeviceSoA &src, int nonfloor_only, double level, unsigned long long *dev_counts256, hipStream_t s) {
    (void)hipMemsetAsync(dev_counts256, 0, 256 * sizeof(unsigned long long), s);
    if (!src.npoints) return;
    CW_LAUNCH("tile_histogram", tile_hist_kernel, dim3(stream_grid(src.npoints)), dim3(FBLOCK), 0, s, nonfloor_only, level, src.y(), src.rgbt(), src.npoints,
              dev_counts256);
}

// ---------------------------------------------------------------------------
// e. bounds: min and max per coordinate, NaN skipped per coordinate
// ---------------------------------------------------------------------------
// (The point grid's box, kernels_grid.hip, leaves out every point that has any non-finite coordinate: it sizes a grid.  The
// analyze filter's comparisons look at one coordinate at a time and take an infinity for what it is.)
__global__ void __launch_bounds__(FBLOCK) bounds_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                       float *__restrict__ partial /* [gridDim.x][6] */) {
    __shared__ float red[6][FWAVES];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t tile = blockIdx.x; tile * FTILE < n; tile += gridDim.x) {
        const size_t base = tile * FTILE + (size_t)threadIdx.x * FITEMS;
        if (base >= n) continue;
        float v[3][FITEMS];
        load_items<float4>(x, base, n, NAN, v[0]);
        load_items<float4>(y, base, n, NAN, v[1]);
        load_items<float4>(z, base, n, NAN, v[2]);
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int j = 0; j < FITEMS; j++) { lo[a] = fminf(lo[a], v[a][j]); hi[a] = fmaxf(hi[a], v[a][j]); }
    }
    for (int a = 0; a < 3; a++) {
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64));
        }
        if ((threadIdx.x & 63) == 0) { red[a][threadIdx.x >> 6] = lo[a]; red[3 + a][threadIdx.x >> 6] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = red[threadIdx.x][0];
        for (int w = 1; w < FWAVES; w++) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
        partial[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}

unsigned bounds_blocks(size_t n) { return n ? (stream_grid(n) > 256 ? 256 : stream_grid(n)) : 0; }

void bounds_partial(const DeviceSoA &src, float *partial, hipStream_t s) {
    const unsigned nb = bounds_blocks(src.npoints);
    if (!nb) return;
    CW_LAUNCH("bounds", bounds_kernel, dim3(nb), dim3(FBLOCK), 0, s, src.x(), src.y(), src.z(), src.npoints, partial);
}

}  // namespace k
}  // namespace cwipc_amd
