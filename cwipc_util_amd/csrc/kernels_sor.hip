// kernels_sor.hip -- statistical outlier removal on gfx950.
//
// Reference: cwipc_remove_outliers, src/cwipc_filters.cpp:181-278; the filter
// itself is pcl::StatisticalOutlierRemoval [PCL upstream], restated in
// oracle/cwipc_oracle.c (sor_filter):
//   d_i  = float( sum_{j=1..k} sqrtf(dist2_j) / k )   exact k+1 nearest (self = j 0),
//          dist2 in fp32 as FLANN's L2_Simple ((dx*dx + dy*dy) + dz*dz), ascending, sum in f64
//   mean / variance over all d_i in f64 (squares formed in fp32), threshold = mean + mul*stddev
//   keep point i iff !(d_i > threshold), input order preserved.
//
// The k nearest distances of a point are a well-defined multiset, so d_i does not
// depend on how the neighbour search is organised.  Here: points are bucketed
// into a uniform grid (kernels_grid.hip; the shell search's parts: point_grid.hpp), each lane
// searches growing cubic shells of cells around its point -- its own row of cells first, rows that can
// no longer hold one of the k + 1 nearest skipped -- and keeps the k + 1 smallest distances as a sorted list
// in registers (insert = one v_med3 per slot; k <= 32; an LDS list up to k = 120); a shell
// radius r proves exactness once the (k+1)-th distance is <= r*h.
#include "point_grid.hpp"

#include <cstdlib>
#include <mutex>
#include <vector>

namespace cwipc_amd {

namespace {
// ---- exact k-NN mean distance ----
// One lane per point (in cell order, so a wave's lanes search the same shells).
// best[] lives in LDS, one column per lane: best[j * QB + lane].
__global__ void __launch_bounds__(QB) knn_mean_dist_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted, size_t n,
                                                          const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count, int k,
                                                          float *__restrict__ dist_out, float *__restrict__ scratch) {
    const GridRows<false> rows(gv, gm, cell_start, cell_count, nullptr);
    const Grid &g = rows.g;
    extern __shared__ float best_all[];
    // the lists live in LDS while (k + 1) x 128 floats fit there (k <= 319), in a slab of device memory per workgroup beyond
    // (the reference takes any k: src/cwipc_filters.cpp:197-201); the workgroups walk over the query tiles
    float *best = scratch ? scratch + (size_t)blockIdx.x * (size_t)(k + 1) * QB + threadIdx.x : best_all + threadIdx.x;
    const int want = k + 1;
    for (size_t tile = blockIdx.x; tile * QB < n; tile += gridDim.x) {
    size_t qi = tile * QB + threadIdx.x;
    if (qi >= n) continue;
    const float4 q = sorted[qi];
    const int cx = cell_coord(g, q.x, 0), cy = cell_coord(g, q.y, 1), cz = cell_coord(g, q.z, 2);
    int have = 0;
    float worst = -1.0f;   // largest of the kept distances
    int worst_at = 0;
    const int maxring = max(g.dim[0], max(g.dim[1], g.dim[2]));
    for (int ring = 0; ring <= maxring; ring++) {
        for (int dz = -ring; dz <= ring; dz++) {
            const int z = cz + dz;
            if (z < 0 || z >= g.dim[2]) continue;
            for (int dy = -ring; dy <= ring; dy++) {
                const int y = cy + dy;
                if (y < 0 || y >= g.dim[1]) continue;
                const bool face = dz == -ring || dz == ring || dy == -ring || dy == ring;
                const int step = face ? 1 : (ring > 0 ? 2 * ring : 1);
                for (int dx = -ring; dx <= ring; dx += step) {
                    const int x = cx + dx;
                    if (x < 0 || x >= g.dim[0]) continue;
                    uint32_t first, last;
                    rows.range(x, x, y, z, first, last);
                    for (uint32_t e = first; e < last; e++) {
                        const float d2 = flann_dist2(q, sorted[e]);
                        if (have < want) {
                            best[have * QB] = d2;
                            if (d2 > worst) { worst = d2; worst_at = have; }
                            have++;
                        } else if (d2 < worst) {
                            best[worst_at * QB] = d2;
                            worst = -1.0f;
                            for (int j = 0; j < want; j++) {
                                float v = best[j * QB];
                                if (v > worst) { worst = v; worst_at = j; }
                            }
                        }
                    }
                }
            }
        }
        if (have == want && shell_proves(g, ring, worst)) break;
    }
    // ascending order, then the f64 sum of fp32 square roots, skipping the query itself
    for (int a = 1; a < have; a++) {
        float v = best[a * QB];
        int b = a;
        while (b > 0 && best[(b - 1) * QB] > v) { best[b * QB] = best[(b - 1) * QB]; b--; }
        best[b * QB] = v;
    }
    double sum = 0.0;
    for (int j = 1; j < have; j++) sum += (double)sqrtf(best[j * QB]);
    dist_out[__float_as_uint(q.w)] = (float)(sum / (double)k);
    }
}

// Launch of the list variant: LDS for the lists as long as they fit (64 KB by default, up to 160 KB once the limit has been
// raised), a slab of device memory per workgroup beyond.  `slab` receives the pool block to give back when the kernel is done.
bool launch_knn_list(const Grid &gv, const GridMeta *gm, const float4 *sorted, size_t n, const uint32_t *cell_start, const uint32_t *cell_count, int k,
                     float *dist_out, hipStream_t s, void **slab) {
    *slab = nullptr;
    const unsigned qgrid = (unsigned)((n + QB - 1) / QB);
    const size_t shmem = (size_t)(k + 1) * QB * sizeof(float);
    // (a device whose LDS limit cannot be raised that far -- the attribute call fails, or the device reports less -- takes the slab
    // path below for these k as well: any kNeighbors works, as in the reference)
    bool in_lds = shmem <= (size_t)160 * 1024 - 512;
    if (in_lds && shmem > (size_t)64 * 1024) {
        static std::mutex once;
        static int raised_on = -1, refused_on = -1;
        std::lock_guard<std::mutex> g(once);
        const int dev = current_device();
        if (refused_on == dev) {
            in_lds = false;
        } else if (raised_on != dev) {
            int lds_max = 0;
            if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) { (void)hipGetLastError(); lds_max = 0; }
            if (lds_max >= 160 * 1024 - 512 &&
                hipFuncSetAttribute(reinterpret_cast<const void *>(&knn_mean_dist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512) == hipSuccess) {
                raised_on = dev;
            } else {
                (void)hipGetLastError();
                refused_on = dev;
                in_lds = false;
            }
        }
    }
    if (in_lds) {
        CW_LAUNCH("sor_knn_mean_dist", knn_mean_dist_kernel, dim3(qgrid), dim3(QB), shmem, s, gv, gm, sorted, n, cell_start, cell_count, k, dist_out, (float *)nullptr);
        return true;
    }
    unsigned blocks = std::min(qgrid, 1024u);
    while (blocks > 64 && (size_t)blocks * shmem > ((size_t)4 << 30)) blocks /= 2;
    if ((size_t)blocks * shmem > ((size_t)16 << 30)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_remove_outliers", "kNeighbors is too large for the device memory the candidate lists would take");
        return false;
    }
    float *scratch = (float *)pool_alloc((size_t)blocks * shmem);
    if (!scratch) return false;
    *slab = scratch;
    CW_LAUNCH("sor_knn_mean_dist", knn_mean_dist_kernel, dim3(blocks), dim3(QB), 0, s, gv, gm, sorted, n, cell_start, cell_count, k, dist_out, scratch);
    return true;
}

// (Round 3, measured: a camera tile's 36 k queries take this kernel 39 us whether they sit 64 or 16 to a wave (567 or 2266 waves
// on 1024 SIMDs): a query is ONE lane's chain of dependent loads -- row lookups, candidates four at a time -- and the kernel lasts
// as long as such a chain, however many run side by side.  Eight candidate loads in flight instead of four: 41 us, no change
// either (sixteen, through an array the compiler put into scratch memory: 149 us).  FOUR LANES PER QUERY (each scans every fourth
// candidate into a list of its own, the lists merged by two butterfly steps over the quad, rows and rings turned away on a bound
// the quad shares; d_i bit-identical, all tests green): 50 us.  The rows of a ring beyond the first looked up eight at a time
// instead of one after the other: 44 us.  So it is neither the candidates nor the row lookups one by one: per wave the counters
// say 4400 vector instructions (7 us), 182 loads and 52 % of 22 us waiting, the slowest waves twice that; what the waves wait
// for is not a cold L2 either (the arrays have just been written from all eight XCDs, but the same kernel launched a second
// time right behind the first takes 37.8 us against 42.4).  Not resolved in round 3.)
// The same search with the candidate list in registers (k + 1 <= KCAP): a sorted list kept by a
// compare-exchange chain, no LDS round trips per accepted candidate.  Unused leading slots hold -inf,
// so the largest kept distance is always the last register.
// SPARSE: cell_start is indexed by the cells that exist (one entry more than there are cells: the end), cell_count is the
// segment table (seg_pack_kernel).
// (r4, second session: six waves per SIMD for k <= 16 -- 80 registers, eight of them spilled, and still 6 % faster at 10 M points than five waves without
// a spill: the counters put 54 % of a wave's cycles there into waiting for its loads (SQ_WAIT_ANY; 249 loads, 5300 vector instructions per wave), and what
// hides a wait is another wave.  Eight waves (44 spilled) give it back; requesting the next four candidates before looking at these four changed nothing at
// five waves and cost 8 % at four.  profiles/r04_sor_knn_10m.txt)
template <int KCAP, bool SPARSE>
__global__ void __launch_bounds__(QB) __attribute__((amdgpu_waves_per_eu(KCAP <= 17 ? 6 : 4))) knn_mean_dist_reg_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted, size_t n,
                                                              const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count, int k,
                                                              float *__restrict__ dist_out, const uint32_t *__restrict__ cell_count2 = nullptr) {
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const int want = k + 1, pad = KCAP - want;
    size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    if (qi >= n) return;
    const float4 q = sorted[qi];
    const int cx = cell_coord(g, q.x, 0), cy = cell_coord(g, q.y, 1), cz = cell_coord(g, q.z, 2);
    float best[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; j++) best[j] = j < pad ? -INFINITY : INFINITY;
    int have = 0;
    // one candidate: its distance, sorted insert (which was most of this kernel's instruction count before it was a median per slot)
    auto candidate = [&](const float4 p) {
        const float d2 = flann_dist2(q, p);
        if (d2 < best[KCAP - 1]) {
            have++;
            sorted_insert(best, d2);
        }
    };
    auto scan = [&](uint32_t first, uint32_t last) { scan_range<1>(sorted, first, last, candidate); };
    auto worst = [&]() { return best[KCAP - 1]; };
    // rings 0 and 1 together: 9 rows, their index loads issued before any of them is needed
    {
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
        uint32_t first[9], last[9];
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int y = cy + (r % 3) - 1, z = cz + (r / 3) - 1;
            first[r] = last[r] = 0;
            if (y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2]) rows.range(x0, x1, y, z, first[r], last[r]);
        }
        // the query's own row first; then a row only if it can still hold one of the k + 1 nearest: its nearest edge must be
        // closer than the worst distance kept so far (near_gap)
        const float eps = (float)(g.h * 1e-5), hf = (float)g.h;
        const float ylo = (float)((double)g.mn[1] + (double)cy * g.h), zlo = (float)((double)g.mn[2] + (double)cz * g.h);
        scan(first[4], last[4]);
        // (rows that share a face with the query's row before the diagonal ones: the sooner the list holds near points,
        // the more rows and candidates the bound turns away)
        constexpr int order[8] = {1, 3, 5, 7, 0, 2, 6, 8};
#pragma unroll
        for (int o = 0; o < 8; o++) {
            const int r = order[o];
            if (near_gap(q.y, ylo, hf, eps, r % 3 - 1) + near_gap(q.z, zlo, hf, eps, r / 3 - 1) >= best[KCAP - 1]) continue;
            scan(first[r], last[r]);
        }
    }
    const int maxring = max(g.dim[0], max(g.dim[1], g.dim[2]));
    for (int ring = 1; ring <= maxring; ring++) {
        if (ring > 1) walk_shell(rows, q, cx, cy, cz, ring, worst, false, scan);   // (shells 0 and 1: above)
        if (have >= want && shell_proves(g, ring, best[KCAP - 1])) break;
    }
    // the f64 sum of fp32 square roots in ascending order, skipping the query itself (the smallest)
    double sum = 0.0;
#pragma unroll
    for (int j = 1; j < KCAP; j++) {
        if (j > pad && best[j] < INFINITY) sum += (double)sqrtf(best[j]);
    }
    dist_out[__float_as_uint(q.w)] = (float)(sum / (double)k);
}

// ---- two lanes per query (r4, second session): small clouds, k = 16 ----
// A camera tile's 36 k queries are half a wave per SIMD: the kernel lasts as long as ONE query's chain -- ~76 candidates four at a time, a sorted insert
// for most of them -- however many queries run side by side.  Here two neighbouring lanes share a query: the same rows, the same ranges, but lane h takes
// every second candidate (first + h, + 2, ...) into a sorted list of its own, so the chain is half as long.  What made round 3's four-lane version slower
// (50 against 39 us) was merging the lists as sorted lists, 17 inserts per butterfly step; a query needs less:
//   * the k + 1 nearest of the pair's candidates are, as a SET, c[j] = min(a[j], b[16 - j]) over the two sorted lists (the first step of a bitonic merge):
//     seventeen DPP swaps and minima, and (k + 1)-th distance so far = max_j c[j] -- the bound that turns rows, rings and candidates away, refreshed
//     after the query's own row, after the face rows and at every ring's end;
//   * d_i = the f64 sum of the sixteen square roots in ascending order, and an f64 sum of seventeen fp32 values whose exponents lie within 2^23 of each
//     other is EXACT in any order (every partial sum is a multiple of the smallest term's unit below 2^53 of it): the set is summed as it stands, minus
//     the smallest term (the query itself); a query whose distances spread further (coincident points next to far ones) sorts its set first.
// Same d_i bit for bit (the outlier tests run through this kernel for k = 16 on small clouds).  Dense layout only, k + 1 = 17.
__device__ __forceinline__ float pair_swap(float v) {   // the other lane of the pair's value (quad_perm [1, 0, 3, 2])
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));
}
__device__ __forceinline__ int pair_swap_i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true); }

__global__ void __launch_bounds__(QB) knn_pair_kernel(const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted, size_t n, const uint32_t *__restrict__ cell_start,
                                                     const uint32_t *__restrict__ cell_count, const uint32_t *__restrict__ cell_count2, float *__restrict__ dist_out) {
    constexpr int KCAP = 17, k = 16;
    const GridRows<false> rows(Grid{}, gm, cell_start, cell_count, cell_count2);   // (gm: never nullptr here)
    const Grid &g = rows.g;
    const size_t qi0 = ((size_t)blockIdx.x * QB + threadIdx.x) >> 1;
    const uint32_t half = threadIdx.x & 1u;
    const bool real = qi0 < n;
    const size_t qi = real ? qi0 : n - 1;   // (lanes beyond the cloud run the last query along, so that every pair is whole: they write nothing)
    const float4 q = sorted[qi];
    const int cx = cell_coord(g, q.x, 0), cy = cell_coord(g, q.y, 1), cz = cell_coord(g, q.z, 2);
    float best[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; j++) best[j] = INFINITY;
    int have = 0;
    float thr = INFINITY;   // nothing at this distance or beyond can be among the pair's k + 1 nearest
    auto candidate = [&](const float4 p) {
        const float d2 = flann_dist2(q, p);
        if (d2 < thr) {
            have++;
            sorted_insert(best, d2);
            thr = fminf(thr, best[KCAP - 1]);
        }
    };
    // this lane's half of a range: first + half, every second one
    auto scan = [&](uint32_t first, uint32_t last) { scan_range<2>(sorted, first + half, last, candidate); };
    auto bound = [&]() { return thr; };
    // the pair's (k + 1)-th distance so far, from the two lists
    auto refresh = [&]() {
        float mk = -INFINITY;
#pragma unroll
        for (int j = 0; j < KCAP; j++) mk = fmaxf(mk, fminf(best[j], pair_swap(best[KCAP - 1 - j])));
        thr = fminf(thr, mk);
    };
    {
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
        uint32_t first[9], last[9];
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int y = cy + (r % 3) - 1, z = cz + (r / 3) - 1;
            first[r] = last[r] = 0;
            if (y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2]) rows.range(x0, x1, y, z, first[r], last[r]);
        }
        const float eps = (float)(g.h * 1e-5), hf = (float)g.h;
        const float ylo = (float)((double)g.mn[1] + (double)cy * g.h), zlo = (float)((double)g.mn[2] + (double)cz * g.h);
        scan(first[4], last[4]);
        refresh();
        constexpr int order[8] = {1, 3, 5, 7, 0, 2, 6, 8};
#pragma unroll
        for (int o = 0; o < 8; o++) {
            const int r = order[o];
            if (o == 4) refresh();
            if (near_gap(q.y, ylo, hf, eps, r % 3 - 1) + near_gap(q.z, zlo, hf, eps, r / 3 - 1) >= thr) continue;
            scan(first[r], last[r]);
        }
    }
    const int maxring = max(g.dim[0], max(g.dim[1], g.dim[2]));
    for (int ring = 1; ring <= maxring; ring++) {
        if (ring > 1) walk_shell(rows, q, cx, cy, cz, ring, bound, false, scan);
        refresh();
        // (both lanes of a pair hold the same thr and the same sum of `have`: they leave together)
        if (have + pair_swap_i(have) >= KCAP && shell_proves(g, ring, thr)) break;
    }
    // the pair's k + 1 nearest as a set
    float c[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; j++) c[j] = fminf(best[j], pair_swap(best[KCAP - 1 - j]));
    float smallest = INFINITY, largest = 0.f, least = INFINITY;   // least: the smallest distance that is not zero
#pragma unroll
    for (int j = 0; j < KCAP; j++) {
        smallest = fminf(smallest, c[j]);
        if (c[j] < INFINITY) largest = fmaxf(largest, c[j]);
        if (c[j] > 0.f) least = fminf(least, c[j]);
    }
    const bool exact = !(least < INFINITY) || sqrtf(largest) < sqrtf(least) * 8388608.f;
    double sum = 0.0;
    if (__builtin_expect(__ballot(!exact) != 0ull, 0)) {
        // distances spread over more than 2^23: the order of the sum may matter -- ascending, as the reference has it
        float srt[KCAP];
#pragma unroll
        for (int j = 0; j < KCAP; j++) srt[j] = INFINITY;
#pragma unroll 1
        for (int i = 0; i < KCAP; i++) {
            float v = c[0];
#pragma unroll
            for (int j = 1; j < KCAP; j++) v = i == j ? c[j] : v;
            sorted_insert(srt, v);
        }
#pragma unroll
        for (int j = 1; j < KCAP; j++) if (srt[j] < INFINITY) sum += (double)sqrtf(srt[j]);
    } else {
#pragma unroll
        for (int j = 0; j < KCAP; j++) if (c[j] < INFINITY) sum += (double)sqrtf(c[j]);
        if (smallest < INFINITY) sum -= (double)sqrtf(smallest);
    }
    if (real && half == 0u) dist_out[__float_as_uint(q.w)] = (float)(sum / (double)k);
}

// (Round 4, built, measured and taken out again -- the commit before this comment's has the kernels, profiles/r04_sor_knn_staged.txt the figures:
// the neighbourhood of 64 consecutive sorted points staged in LDS by the whole wave -- the nine runs of cells [ca - 1, cb + 1] shifted by the row
// offsets, one round trip -- and every lane scanning its own three cells of each row there; before it, a wave per row of cells.  d_i bit-identical;
// 43.0 us against 42.3 for a 36 k-point camera tile, the same at every cell size from 4 to 50 points per cell (a wave per row: 61-67 us).  The
// kernel does not wait for its candidates: its time is the sorted insert -- 17 medians, run by the whole wave whenever ONE lane accepts, ~1400 of
// ~4400 vector instructions per wave at one wave per SIMD -- and the second ring of the queries at the cloud's edge, which every wave has.)

// ---- mean / variance, deterministic two-level sum ----
__global__ void __launch_bounds__(GRID_BLK) stats_partial_kernel(const float *__restrict__ d, size_t n, double *__restrict__ partial) {
    __shared__ double red[2][GRID_BLK / 64];
    double s = 0, q = 0;
    // contiguous slice per workgroup, strided by lane inside it: fixed order for a fixed launch shape
    size_t per = (n + gridDim.x - 1) / gridDim.x;
    size_t lo = (size_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    for (size_t i = lo + threadIdx.x; i < hi; i += GRID_BLK) {
        float v = d[i];
        s += (double)v;
        q += (double)__fmul_rn(v, v);   // "distance * distance" is an fp32 product upstream
    }
    for (int off = 32; off > 0; off >>= 1) {   // (two sums a step)
        s += __shfl_down(s, off, 64);
        q += __shfl_down(q, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0, tq = 0;
        for (int w = 0; w < GRID_BLK / 64; w++) { ts += red[0][w]; tq += red[1][w]; }
        partial[2 * blockIdx.x] = ts;
        partial[2 * blockIdx.x + 1] = tq;
    }
}

// The outlier filter's search on the grid (a GridSearch): d_i into dev_dist -- candidate lists in registers up to k + 1 = 33
// (small clouds' flow, the one that gives counts2, with k = 16: two lanes per query), beyond that launch_knn_list, which reads
// the dense layout without counts2 only.  False: the search failed.
bool launch_knn(const GridView &v, int k, float *dev_dist, hipStream_t s) {
    static const bool pair_off = []() { const char *e = getenv("CWIPC_SOR_PAIR"); return e && atoi(e) == 0; }();   // test knob: a lane per query
    const unsigned qgrid = (unsigned)((v.n + QB - 1) / QB);
    if (v.counts2 && k == 16 && !pair_off) {
        CW_LAUNCH("sor_knn_mean_dist", knn_pair_kernel, dim3((unsigned)((2 * v.n + QB - 1) / QB)), dim3(QB), 0, s, v.gm, v.sorted, v.n, v.starts, v.counts, v.counts2, dev_dist);
    } else if (k + 1 <= 17 && v.sparse) {
        CW_LAUNCH("sor_knn_mean_dist", (knn_mean_dist_reg_kernel<17, true>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, k, dev_dist, v.counts2);
    } else if (k + 1 <= 17) {
        CW_LAUNCH("sor_knn_mean_dist", (knn_mean_dist_reg_kernel<17, false>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, k, dev_dist, v.counts2);
    } else if (k + 1 <= 33 && v.sparse) {
        CW_LAUNCH("sor_knn_mean_dist", (knn_mean_dist_reg_kernel<33, true>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, k, dev_dist, v.counts2);
    } else if (k + 1 <= 33) {
        CW_LAUNCH("sor_knn_mean_dist", (knn_mean_dist_reg_kernel<33, false>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.n, v.starts, v.counts, k, dev_dist, v.counts2);
    } else {   // (sor_mean_distances asks for the dense layout for these k)
        void *slab = nullptr;
        const bool ok = launch_knn_list(v.g, v.gm, v.sorted, v.n, v.starts, v.counts, k, dev_dist, s, &slab);
        tctx().free_later(slab);
        return ok;
    }
    return true;
}

}  // namespace

bool sor_mean_distances(const DeviceSoA &src, int k, float *dev_dist) {
    if (k < 1) {
        ThreadCtx &c = tctx();
        if (!c.ensure()) return false;
        if (src.npoints == 0) return true;
        CW_HIP_TRY(hipMemsetAsync(dev_dist, 0, src.npoints * sizeof(float), c.stream));
        return c.sync();
    }
    // (any k, as the reference: lists in registers up to k = 32, in LDS up to k = 319, in device memory beyond: launch_knn_list)
    const GridSearch search = [&](const GridView &v, hipStream_t s) { return launch_knn(v, k, dev_dist, s); };
    return grid_and_search(src, k, k + 1 <= 33, search);
}

// mean, variance and threshold from the 1024 partial sums: a pairwise tree (s[i] = s[2i] + s[2i+1], ten
// levels), the order the host version (sor_threshold) follows too, then the same f64 expressions
__global__ void __launch_bounds__(1024) stats_final_kernel(const double *__restrict__ partial, size_t n, float stddev_mul, double *__restrict__ thr) {
    __shared__ double s[1024], q[1024];
    s[threadIdx.x] = partial[2 * threadIdx.x];
    q[threadIdx.x] = partial[2 * threadIdx.x + 1];
    __syncthreads();
    for (unsigned width = 512; width >= 1; width >>= 1) {
        double a = 0, b = 0;
        if (threadIdx.x < width) { a = s[2 * threadIdx.x] + s[2 * threadIdx.x + 1]; b = q[2 * threadIdx.x] + q[2 * threadIdx.x + 1]; }
        __syncthreads();
        if (threadIdx.x < width) { s[threadIdx.x] = a; q[threadIdx.x] = b; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double sum = s[0], sq_sum = q[0];
    const double valid = (double)n;
    const double mean = sum / valid;
    const double variance = (sq_sum - sum * sum / valid) / (valid - 1);
    const double stddev = sqrt(variance);
    *thr = mean + (double)stddev_mul * stddev;
}

// (Both in one launch -- the workgroup that takes the last ticket runs the tree -- was built and measured in round 3: 29 us with a
// ticket per partial sum, 16 us with sixteen partial sums per workgroup and ticket, against 3 + 3 us for the two kernels and the
// boundary between them.  A compaction's count and scan in one launch do pay: kernels_basic.hip.)
bool sor_threshold_device(const float *dev_dist, size_t n, float stddev_mul, double *thr_dev) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const unsigned nb = 1024;
    double *partial = (double *)pool_alloc(nb * 2 * sizeof(double));
    if (!partial) return false;
    CW_LAUNCH("sor_stats", stats_partial_kernel, dim3(nb), dim3(GRID_BLK), 0, c.stream, dev_dist, n, partial);
    CW_LAUNCH("sor_stats_final", stats_final_kernel, dim3(1), dim3(1024), 0, c.stream, partial, n, stddev_mul, thr_dev);   // nb == 1024
    c.free_later(partial);
    return hipGetLastError() == hipSuccess;
}

bool sor_threshold(const float *dev_dist, size_t n, float stddev_mul, double *thr) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const unsigned nb = 1024;
    double *partial = (double *)pool_alloc(nb * 2 * sizeof(double));
    if (!partial) return false;
    CW_LAUNCH("sor_stats", stats_partial_kernel, dim3(nb), dim3(GRID_BLK), 0, c.stream, dev_dist, n, partial);
    double *h = (double *)c.staging(nb * 2 * sizeof(double));
    bool ok = h && hipMemcpyAsync(h, partial, nb * 2 * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(partial);
    if (!ok) return false;
    // pairwise tree over the partial sums, as stats_final_kernel does it
    std::vector<double> s(nb), q(nb);
    for (unsigned b = 0; b < nb; b++) { s[b] = h[2 * b]; q[b] = h[2 * b + 1]; }
    for (unsigned width = nb / 2; width >= 1; width >>= 1)
        for (unsigned i = 0; i < width; i++) { s[i] = s[2 * i] + s[2 * i + 1]; q[i] = q[2 * i] + q[2 * i + 1]; }
    const double sum = s[0], sq_sum = q[0];
    // pcl::StatisticalOutlierRemoval: every point is "valid" here (finite input)
    double valid = (double)n;
    double mean = sum / valid;
    double variance = (sq_sum - sum * sum / valid) / (valid - 1);
    double stddev = sqrt(variance);
    *thr = mean + (double)stddev_mul * stddev;
    return true;
}

std::shared_ptr<DeviceSoA> sor_threshold_and_select(const DeviceSoA &src, const float *dev_dist, float stddev_mul, double *thr_dev) {
    const size_t n = src.npoints;
    static const bool fold_off = []() { const char *e = getenv("CWIPC_SOR_STATS_FOLD"); return e && atoi(e) == 0; }();   // test knob: the statistics' second kernel on its own
    if (n > k::compact_small_cloud_limit() || fold_off) {
        if (!sor_threshold_device(dev_dist, n, stddev_mul, thr_dev)) return nullptr;
        return sor_select(src, dev_dist, 0.0, thr_dev);
    }
    // small clouds: the partial sums only; the compaction's count kernel turns them into the threshold (kernels_basic.hip, threshold_from_partials)
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    const unsigned nb = 1024;
    double *partial = (double *)pool_alloc(nb * 2 * sizeof(double));
    if (!partial) return nullptr;
    CW_LAUNCH("sor_stats", stats_partial_kernel, dim3(nb), dim3(GRID_BLK), 0, c.stream, dev_dist, n, partial);
    k::Predicate p{};
    p.mode = 3;
    p.dist = dev_dist;
    p.thr_dev = thr_dev;
    p.stat_partial = partial; p.stat_n = n; p.stat_mul = stddev_mul; p.thr_out = thr_dev;
    auto out = compact(src, p);   // (waits for its kernels)
    c.free_later(partial);
    return out;
}

std::shared_ptr<DeviceSoA> sor_select(const DeviceSoA &src, const float *dev_dist, double thr, const double *thr_dev) {
    k::Predicate p{};
    p.mode = 3;
    p.dist = dev_dist;
    p.thr = thr;
    p.thr_dev = thr_dev;
    return compact(src, p);   // (waits for its kernels: the caller frees dev_dist afterwards)
}

}  // namespace cwipc_amd
