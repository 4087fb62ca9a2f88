// block_scan.hpp -- the one-workgroup exclusive scan of per-workgroup counts that every stable compaction here ends its count pass
// with (kernels_basic.hip: tilefilter, crop, outlier removal; kernels_rgbd.hip: the RGB-D source).  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cwipc_amd {
namespace k {

// The exclusive scan of the block counts by the workgroup that runs it (NT lanes): counts[i] <- sum of those before, counts[nblocks]
// <- the total, which also goes to a pinned host word with `tag` in its upper half (one 64-bit store, no fence: the host polls for
// the tag instead of waiting for the stream).
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
        uint32_t inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
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
        counts[nblocks] = carry;   // for the scatter kernel: a compaction that keeps every point moves nothing
        __hip_atomic_store(total, ((unsigned long long)tag << 32) | carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace k
}  // namespace cwipc_amd
