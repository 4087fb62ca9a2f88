// kernels_cluster.hip -- gfx950 kernels of cwipc_hip_clusters and cwipc_hip_cluster_filter: Euclidean cluster extraction, the
// connected components of "closer than radius" (RULE K of include/cwipc_util_amd/hip_ext.h has the contract in full;
// tests/cluster_model.py is its numpy and scipy model).
//
//   link     one lane per point of the point grid's sorted array (grid_and_search, any of its three flows).  walk_exact with the
//            constant limit r2 is an exact fixed-radius search: its bounds never turn away a cell that holds a point AT the limit,
//            let alone under it.  Every candidate j with d2 < r2 (the f64 arithmetic of cwipc_hip_correspondences, strictly) and,
//            under SAME_TILE, an equal tile byte, is united with the lane's point i in the atomic union-find of union_find.hpp --
//            over ORIGINAL indices, so a root is a component's smallest original index whatever the grid did with the points.
//            Each unordered pair is united once, by the lane of its larger index.  A lane remembers a value from its own chain of
//            parents (what its last union returned) and skips a candidate whose word equals it: in a dense clump nearly every
//            candidate after the first few already hangs under the clump's root.
//   roots    root[i] = find(i), 0xFFFFFFFF for a point with a non-finite coordinate; flag[i] = (root[i] == i); the component's
//            point count by integer atomics into its root's word, one atomic per run of equal roots in a wave.
//   scan     exclusive scan of the flags: a root's cluster number -- clusters are numbered in ascending order of root -- and,
//            behind the last flag, the number of clusters.
//   label    label[i] = number[root[i]]; sizes[number[r]] = the count of root r.
//   rank     (max_clusters > 0 only) the max_clusters-th largest size T by four passes of 8-bit radix selection over the sizes,
//            as the floor helpers select their radii (kernels_floor.hip); the clusters of size T are ranked among themselves by
//            an exclusive scan of (size == T) over the cluster numbers, and the first `need` of them stay.
//   keep     drop[i] = 0 (keep) or 1: the float plane that the outlier filter's stable compaction takes (sor_select, as the
//            direction filter feeds it).
// Sizes come from integer atomics and every other step is a function of the partition, so nothing in the result depends on the
// grid's layout, the launch shape or the order in which lanes ran.
#include "point_grid.hpp"
#include "block_scan.hpp"
#include "union_find.hpp"

#include <algorithm>
#include <type_traits>
#include <rocprim/device/device_scan.hpp>

namespace cwipc_amd {

namespace {

constexpr uint32_t CL_NONE = 0xFFFFFFFFu;
constexpr int CL_GRID_WIDTH = 15;   // the grid's cell size: as for nn_distance2 and the ICP searches (about eight points to an occupied cell)

// the device's atomics, counting a find's loads (link statistics: cwipc_hip_cluster_link_stats)
struct UfCountingAtomics {
    uint32_t loads = 0;
    __device__ __forceinline__ uint32_t load(const uint32_t *p) { loads++; return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t fetch_min(uint32_t *p, uint32_t v) { return atomicMin(p, v); }
};

struct LinkArgs {
    uint32_t *parent;            // n words, parent[i] = i before the launch
    const uint32_t *rgbt;        // the cloud's colour / tile words, original order
    double r2;
    int same_tile;
    unsigned long long *stats;   // nullptr, or 4 words: links seen (j < i) | unions issued | parent words loaded | most loaded by one union
};

__global__ void __launch_bounds__(GRID_BLK) cluster_init_kernel(uint32_t *__restrict__ parent, uint32_t *__restrict__ rootsize, size_t n) {
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) {
        parent[i] = (uint32_t)i;
        rootsize[i] = 0;
    }
}

template <bool SPARSE, bool STATS>
__global__ void __launch_bounds__(QB) cluster_link_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted, size_t n,
                                                         const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count,
                                                         const uint32_t *__restrict__ cell_count2, LinkArgs A) {
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    unsigned long long links = 0, unions = 0, loads = 0, deepest = 0;
    if (qi < n) {
        const float4 me = sorted[qi];
        if (isfinite(me.x) && isfinite(me.y) && isfinite(me.z)) {
            const uint32_t i = __float_as_uint(me.w);
            const double q[3] = {(double)me.x, (double)me.y, (double)me.z};
            const int c[3] = {cell_coord(g, me.x, 0), cell_coord(g, me.y, 1), cell_coord(g, me.z, 2)};
            const uint32_t tile_i = A.same_tile ? A.rgbt[i] >> 24 : 0u;
            typename std::conditional<STATS, UfCountingAtomics, UfDeviceAtomics>::type at;
            uint32_t under = i;   // a value from i's own chain of parents: whatever hangs directly under it is in i's component
            auto limit = [&]() { return A.r2; };
            auto candidate = [&](const float4 p) {
                const uint32_t j = __float_as_uint(p.w);
                if (j >= i) return;   // the pair's larger index unites it (and i is no neighbour of itself)
                const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 < A.r2)) return;   // (a candidate with a non-finite coordinate: inf or NaN, never under the limit)
                if (A.same_tile && (A.rgbt[j] >> 24) != tile_i) return;
                if (STATS) links++;
                if (__hip_atomic_load(A.parent + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == under) return;
                if constexpr (STATS) {
                    const uint32_t before = at.loads;
                    under = uf_union(A.parent, i, j, at);
                    unions++;
                    const unsigned long long took = at.loads - before;
                    deepest = took > deepest ? took : deepest;
                } else {
                    under = uf_union(A.parent, i, j, at);
                }
            };
            auto scan = [&](uint32_t first, uint32_t last) { scan_range<1>(sorted, first, last, candidate); };
            walk_exact(rows, q, c, limit, scan);
            if constexpr (STATS) loads = at.loads;
        }
    }
    if constexpr (STATS) {   // every lane of the wave is here
        for (int off = 32; off > 0; off >>= 1) {
            links += __shfl_down(links, off, 64);
            unions += __shfl_down(unions, off, 64);
            loads += __shfl_down(loads, off, 64);
            const unsigned long long o = __shfl_down(deepest, off, 64);
            deepest = o > deepest ? o : deepest;
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(A.stats + 0, links);
            atomicAdd(A.stats + 1, unions);
            atomicAdd(A.stats + 2, loads);
            atomicMax(A.stats + 3, deepest);
        }
    }
}

// root[i], flag[i] (flag[n] = 0: the scan leaves the number of clusters there), and the roots' point counts.  Every lane of a
// wave runs the same number of steps, so the ballots see all 64.
__global__ void __launch_bounds__(GRID_BLK) cluster_roots_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                                uint32_t *parent, uint32_t *__restrict__ root, uint32_t *__restrict__ flag,
                                                                uint32_t *__restrict__ rootsize) {
    const int lane = threadIdx.x & 63;
    UfDeviceAtomics at;
    for (size_t base = (size_t)blockIdx.x * GRID_BLK; base < n + 1; base += (size_t)gridDim.x * GRID_BLK) {
        const size_t i = base + threadIdx.x;
        uint32_t r = CL_NONE;
        if (i < n && isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i])) r = uf_find(parent, (uint32_t)i, at);
        if (i < n) root[i] = r;
        if (i <= n) flag[i] = (i < n && r == (uint32_t)i) ? 1u : 0u;
        // one atomic per set of equal roots in the wave: a cloud that is one cluster would otherwise send every point to one word
        bool todo = r != CL_NONE;
        for (;;) {
            const unsigned long long m = __ballot(todo);
            if (!m) break;
            const int lead = __ffsll((long long)m) - 1;
            const uint32_t lr = (uint32_t)__shfl((int)r, lead, 64);
            const bool mine = todo && r == lr;
            const unsigned long long mm = __ballot(mine);
            if (lane == lead) atomicAdd(&rootsize[lr], (uint32_t)__popcll(mm));
            if (mine) todo = false;
        }
    }
}

__global__ void __launch_bounds__(GRID_BLK) cluster_label_kernel(const uint32_t *__restrict__ root, const uint32_t *__restrict__ number,
                                                                const uint32_t *__restrict__ rootsize, size_t n, uint32_t *__restrict__ label,
                                                                uint32_t *__restrict__ sizes) {
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) {
        const uint32_t r = root[i];
        label[i] = r == CL_NONE ? CL_NONE : number[r];
        if (r == (uint32_t)i) sizes[number[i]] = rootsize[i];
    }
}

// ---- ranking: the max_clusters-th largest size by radix selection.  state: [0] prefix / T  [1] rank still to find / need  [2] 1: every cluster stays
//      [4, 260) the pass's histogram (zero before the first pass; each pick clears it for the next) ----
constexpr int CL_STATE_WORDS = 4 + 256;

__global__ void __launch_bounds__(256) cluster_rank_hist_kernel(int pass, const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ nclusters,
                                                                uint32_t *__restrict__ state) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t C = *nclusters, prefix = pass ? state[0] : 0u;
    const int shift = 24 - 8 * pass;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < C; c += (size_t)gridDim.x * 256) {
        const uint32_t s = sizes[c];
        if (pass == 0 || (s >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&h[(s >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&state[4 + threadIdx.x], h[threadIdx.x]);
}

// one workgroup: the bin, from the top, in which the rank falls.  Among the sizes that share the prefix there are at least as many as
// the rank (max_clusters < C; otherwise state[2] says that every cluster stays and the rest is not read).
__global__ void __launch_bounds__(256) cluster_rank_pick_kernel(int pass, uint32_t max_clusters, const uint32_t *__restrict__ nclusters, uint32_t *__restrict__ state) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = state[4 + threadIdx.x];
    state[4 + threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (pass == 0) { state[0] = 0; state[1] = max_clusters; state[2] = max_clusters >= *nclusters ? 1u : 0u; }
    const uint32_t want = state[1];
    uint32_t above = 0;
    for (int b = 255; b >= 0; b--) {
        if (above + h[b] >= want) {
            state[0] |= (uint32_t)b << (24 - 8 * pass);
            state[1] = want - above;
            break;
        }
        above += h[b];
    }
}

__global__ void __launch_bounds__(GRID_BLK) cluster_rank_flag_kernel(const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ nclusters,
                                                                    const uint32_t *__restrict__ state, size_t n, uint32_t *__restrict__ flag) {
    const uint32_t C = *nclusters, T = state[0];
    for (size_t c = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; c < n + 1; c += (size_t)gridDim.x * GRID_BLK) flag[c] = (c < C && sizes[c] == T) ? 1u : 0u;
}

// drop[i]: 0 keep, 1 drop.  state / equal_rank: nullptr without a limit on the number of clusters.
__global__ void __launch_bounds__(GRID_BLK) cluster_keep_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ sizes, size_t n,
                                                               unsigned long long min_points, const uint32_t *__restrict__ state,
                                                               const uint32_t *__restrict__ equal_rank, float *__restrict__ drop) {
    const bool limited = state != nullptr && state[2] == 0u;
    const uint32_t T = limited ? state[0] : 0u, need = limited ? state[1] : 0u;
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) {
        const uint32_t c = label[i];
        bool keep = false;
        if (c != CL_NONE) {
            const uint32_t s = sizes[c];
            keep = (unsigned long long)s >= min_points && (!limited || s > T || (s == T && equal_rank[c] < need));
        }
        drop[i] = keep ? 0.f : 1.f;
    }
}

template <bool STATS>
void launch_link(const GridView &v, const LinkArgs &A, hipStream_t s) {
    const unsigned qgrid = (unsigned)((v.n + QB - 1) / QB);
    if (v.sparse)
        CW_LAUNCH("cluster_link", (cluster_link_kernel<true, STATS>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, A);
    else
        CW_LAUNCH("cluster_link", (cluster_link_kernel<false, STATS>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, A);
}

// out[0 .. n] = exclusive scan of in[0 .. n] (n + 1 words)
bool scan_words(const uint32_t *in, uint32_t *out, size_t n, ThreadCtx &c) {
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, 0u, n + 1, rocprim::plus<uint32_t>(), c.stream);
    void *tmp = e == hipSuccess ? pool_alloc(tmp_bytes ? tmp_bytes : 256) : nullptr;
    if (e == hipSuccess && !tmp) e = hipErrorOutOfMemory;
    if (e == hipSuccess) {
        if (profiling_enabled()) profile_begin("cluster_scan", c.stream);
        e = rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, n + 1, rocprim::plus<uint32_t>(), c.stream);
        if (profiling_enabled()) profile_end(c.stream);
    }
    c.free_later(tmp);
    if (e != hipSuccess) return hip_failed(e, "rocprim::exclusive_scan", __FILE__, __LINE__);
    return true;
}

size_t round64(size_t words) { return (words + 63) & ~(size_t)63; }

}  // namespace

bool cluster_work_alloc(size_t n, ClusterWork &w) {
    const size_t a = round64(n), b = round64(n + 1);
    const size_t words = 5 * a + 2 * b + round64(CL_STATE_WORDS) + 64;
    w.block = pool_alloc(words * sizeof(uint32_t) + a * sizeof(float));
    if (!w.block) return false;
    uint32_t *p = (uint32_t *)w.block;
    w.n = n;
    w.parent = p; p += a;
    w.root = p; p += a;
    w.rootsize = p; p += a;
    w.sizes = p; p += a;
    w.labels = p; p += a;
    w.flag = p; p += b;
    w.number = p; p += b;
    w.state = p; p += round64(CL_STATE_WORDS);
    w.stats = (unsigned long long *)p; p += 64;
    w.drop = (float *)p;
    w.nclusters = w.number + n;
    return true;
}

bool cluster_labels(const DeviceSoA &src, double r2, bool same_tile, const ClusterWork &w, bool with_stats) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t n = src.npoints;
    if (n == 0 || n != w.n) return false;
    CW_LAUNCH("cluster_init", cluster_init_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, w.parent, w.rootsize, n);
    if (with_stats) CW_HIP_TRY(hipMemsetAsync(w.stats, 0, 4 * sizeof(unsigned long long), c.stream));
    LinkArgs A{};
    A.parent = w.parent;
    A.rgbt = src.rgbt();
    A.r2 = r2;
    A.same_tile = same_tile ? 1 : 0;
    A.stats = with_stats ? w.stats : nullptr;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        if (with_stats) launch_link<true>(v, A, s);
        else launch_link<false>(v, A, s);
        return hipGetLastError() == hipSuccess;
    };
    if (!grid_and_search(src, CL_GRID_WIDTH, true, search)) return false;
    CW_LAUNCH("cluster_roots", cluster_roots_kernel, dim3(grid_blocks(n + 1)), dim3(GRID_BLK), 0, c.stream, src.x(), src.y(), src.z(), n, w.parent, w.root, w.flag,
              w.rootsize);
    if (!scan_words(w.flag, w.number, n, c)) return false;
    CW_LAUNCH("cluster_label", cluster_label_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, w.root, w.number, w.rootsize, n, w.labels, w.sizes);
    return hipGetLastError() == hipSuccess;
}

bool cluster_keep_flags(const ClusterWork &w, uint64_t min_points, uint32_t max_clusters) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t n = w.n;
    const uint32_t *state = nullptr, *equal_rank = nullptr;
    if (max_clusters > 0) {
        CW_HIP_TRY(hipMemsetAsync(w.state, 0, CL_STATE_WORDS * sizeof(uint32_t), c.stream));
        const unsigned hgrid = std::min(1024u, (unsigned)((n + 255) / 256));
        for (int pass = 0; pass < 4; pass++) {
            CW_LAUNCH("cluster_rank_hist", cluster_rank_hist_kernel, dim3(hgrid), dim3(256), 0, c.stream, pass, w.sizes, w.nclusters, w.state);
            CW_LAUNCH("cluster_rank_pick", cluster_rank_pick_kernel, dim3(1), dim3(256), 0, c.stream, pass, max_clusters, w.nclusters, w.state);
        }
        // the flags and, in the words that held the parents, the rank among the clusters of size T (the number of clusters stays in number[n])
        CW_LAUNCH("cluster_rank_flag", cluster_rank_flag_kernel, dim3(grid_blocks(n + 1)), dim3(GRID_BLK), 0, c.stream, w.sizes, w.nclusters, w.state, n, w.flag);
        if (!scan_words(w.flag, w.parent, n > 0 ? n - 1 : 0, c)) return false;
        state = w.state;
        equal_rank = w.parent;
    }
    CW_LAUNCH("cluster_keep", cluster_keep_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, w.labels, w.sizes, n, (unsigned long long)min_points, state,
              equal_rank, w.drop);
    return hipGetLastError() == hipSuccess;
}

}  // namespace cwipc_amd
