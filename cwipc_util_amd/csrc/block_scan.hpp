// block_scan.hpp -- the wave and workgroup sums and scans that every count-scan-scatter here is made of, stated once.  Device code only.
//   wave_inclusive_scan   compact_scatter_kernel (its steps share one barrier), entropy_plan_kernel, entropy_block_decode_kernel,
//                         and the scans below
//   wave_reduce_sum       kernels_grid (cell censuses), kernels_direction (f64 sums), kernels_render, kernels_entropy, block_sum
//   block_sum             count_tile (kernels_basic), codec_popcount_kernel
//   block_exclusive_scan  marker_grey_rows_kernel
//   scan_block_counts     compact_scan_kernel, codec_scan_kernel, codec_decode_scan_kernel, last_block_scans
//   last_block_scans      compact_count_scan_kernel, rgbd_count_scan_kernel
// Written out where they are used: folds that are no sum (min / max, or), __shfl_xor butterflies, loops that fold several values a
// step (a comment at each), wave totals that ballots count (floor_count_kernel, codec_count_kernel, count_tile of kernels_rgbd).
// Kept as they were, because a call changed their code and their times did not stay inside the parent's: floor_scan_kernel (the scan
// once per class), codec_expand_kernel, wave_cumulate (kernels_entropy), the ICP sums' wave sum; and kernels_voxel.hip's copies,
// which must compile to the very instructions they replace.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace cwipc_amd {
namespace k {

// v of this lane and of every lane of its wave in front of it
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// v of lane 0 <- the wave's sum.  The steps run 32, 16, ... 1: for a floating-point T that order is part of the result.  In place,
// as the loops it replaces were (callers reduce the elements of an array in an unrolled loop).
template <class T>
__device__ __forceinline__ void wave_reduce_sum(T &v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
}

// Thread 0's return value: the sum of v over the workgroup's (NT) lanes.  One barrier; wave_lds: NT / 64 words.
template <int NT>
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *wave_lds) {
    wave_reduce_sum(v);
    if ((threadIdx.x & 63) == 0) wave_lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NT / 64; w++) t += wave_lds[w];
    return t;
}

// The sum of v over the workgroup's (NT) lanes in front of this one; *total (may be null) <- the sum over all of them.  One barrier;
// wave_lds: NT / 64 words, not to be written again before another barrier.
template <int NT>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_lds, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v);
    if (lane == 63) wave_lds[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < NT / 64; w++) {
        const uint32_t s = wave_lds[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    if (total) *total = all;
    return before + inc - v;
}

// The exclusive scan of nblocks counts by the one workgroup (NT lanes) that runs it, NT counts a round, the sum so far carried from
// round to round: counts[i] <- the sum of those before, counts[nblocks] <- the total (every point kept: the scatter kernel moves
// nothing), which also goes to a pinned host word with `tag` in its upper half (one 64-bit store, no fence: the host polls for the
// tag instead of waiting for the stream; pinned_report.hpp).
template <int NT>
__device__ __forceinline__ void scan_block_counts(uint32_t *__restrict__ counts, size_t nblocks, unsigned long long *__restrict__ total, uint32_t tag) {
    __shared__ uint32_t wave_tot[NT / 64];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t base = 0; base < nblocks; base += NT) {
        size_t i = base + threadIdx.x;
        uint32_t v = i < nblocks ? counts[i] : 0;
        const uint32_t inc = wave_inclusive_scan(v);
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        uint32_t wave_base = 0;
        for (int w = 0; w < wave; w++) wave_base += wave_tot[w];
        uint32_t c = carry;
        if (i < nblocks) counts[i] = c + wave_base + inc - v;
        __syncthreads();
        if (threadIdx.x == NT - 1) carry = c + wave_base + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[nblocks] = carry;
        __hip_atomic_store(total, ((unsigned long long)tag << 32) | carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Count and scan in one launch.  Every workgroup (NT lanes) brings its count in thread 0, leaves it in counts[blockIdx.x] and takes
// a ticket; the one that takes the last ticket scans all gridDim.x counts as above.  *ticket is 0 before the launch and after it.
// The ordering: thread 0's acq_rel add to the ticket releases its count, stored (relaxed) in front of it.  The adds of all workgroups
// are one release sequence on one word, so the add that reads gridDim.x - 1 synchronises with every other and its acquire half puts
// every count in front of that thread 0; the barrier hands is_last on, and each lane's own acquire fence makes its plain loads of
// counts[] read what was released.  Agent scope: the workgroups run on different compute units and XCDs of one device, which
// workgroup scope does not reach, and nobody outside the device reads the counts.  The reset is relaxed: every ticket is taken.
// Small inputs only: at 10 M points (2441 workgroups) tilefilter went 81 -> 129 us, crop 70 -> 147 -- an agent-scope release
// writes the XCD's L2 back, and all tickets are one address at the memory side.
template <int NT>
__device__ __forceinline__ void last_block_scans(uint32_t my_count, uint32_t *__restrict__ counts, uint32_t *__restrict__ ticket,
                                                 unsigned long long *__restrict__ total_host, uint32_t tag) {
    __shared__ uint32_t is_last;
    if (threadIdx.x == 0) {
        __hip_atomic_store(&counts[blockIdx.x], my_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t before = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        is_last = before == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next kernel that uses it
    scan_block_counts<NT>(counts, gridDim.x, total_host, tag);
}

}  // namespace k
}  // namespace cwipc_amd
