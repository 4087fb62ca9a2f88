// kernels_grid.hip -- the uniform grid over a cloud's points: built here, searched by the client's kernels (point_grid.hpp).
//
// Points are bucketed into a uniform grid by a counting sort (one atomic per run of equal cells in a wave); `sorted` holds them
// in cell order, x fastest.  Two layouts: dense (small and medium clouds; the grid itself -- box, cell size from an occupancy
// census -- is decided by two one-wave kernels on the device, no host round trip), and sparse (from 2^20 points: segments of
// 16 cells along x that exist only where points are, see SEG).  Three flows build them (grid_and_search, at the end); each ends
// by calling the search it was given, on its stream, and gives the grid's arrays back to the pool behind it.
#include "point_grid.hpp"
#include "block_scan.hpp"

#include <cstdlib>
#include <cstring>
#include <rocprim/device/device_scan.hpp>

namespace cwipc_amd {

namespace {

constexpr size_t MAX_CELLS = (size_t)1 << 27;   // dense grid cells at most (three 4-byte arrays of this length); a call uses 8 per point at most

__device__ __forceinline__ void grid_dims(Grid &g, const double ext[3], double h) {
    for (int a = 0; a < 3; a++) g.dim[a] = (int)floor(ext[a] / h) + 1;
    g.h = h;
    g.inv_h = 1.0 / h;
    g.nsegx = (g.dim[0] + SEG - 1) / SEG;
}
__device__ __forceinline__ size_t grid_cells(const Grid &g) { return (size_t)g.dim[0] * (size_t)g.dim[1] * (size_t)g.dim[2]; }

// one wave of the first workgroup: the cloud's box from the partial boxes, then the finest grid of at most cap_cells cells
// ... and the same launch clears the two per-cell arrays of the counting sort (its other workgroups: two memsets less)
__global__ void __launch_bounds__(GRID_BLK) grid_setup_zero_kernel(const float *__restrict__ partial, unsigned nb, size_t cap_cells, GridMeta *__restrict__ m,
                                                             uint32_t *__restrict__ counts, uint32_t *__restrict__ cursor) {
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const size_t nvec = cap_cells / 4;
    uint4 *c4 = reinterpret_cast<uint4 *>(counts), *u4 = reinterpret_cast<uint4 *>(cursor);
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < nvec; i += (size_t)gridDim.x * GRID_BLK) { c4[i] = zero; u4[i] = zero; }
    if (blockIdx.x == 0 && threadIdx.x < (cap_cells & 3)) { counts[nvec * 4 + threadIdx.x] = 0; cursor[nvec * 4 + threadIdx.x] = 0; }
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (unsigned b = threadIdx.x; b < nb; b += 64)
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], partial[b * 6 + a]); hi[a] = fmaxf(hi[a], partial[b * 6 + 3 + a]); }
    for (int a = 0; a < 3; a++)
        for (int off = 32; off > 0; off >>= 1) { lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64)); hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64)); }
    if (threadIdx.x != 0) return;
    Grid g;
    double ext[3], maxext = 0;
    for (int a = 0; a < 3; a++) {
        g.mn[a] = lo[a] == FLT_MAX ? 0.f : lo[a];
        ext[a] = (double)hi[a] - (double)lo[a];
        if (!(ext[a] >= 0)) ext[a] = 0;   // no finite point
        if (ext[a] > maxext) maxext = ext[a];
    }
    if (!(maxext > 0)) maxext = 1.0;
    double h = maxext / 1024.0;
    grid_dims(g, ext, h);
    while (grid_cells(g) > cap_cells) { h *= 1.25; grid_dims(g, ext, h); }
    m->g = g;
    for (int a = 0; a < 3; a++) m->ext[a] = ext[a];
    m->maxext = maxext;
    m->occ = 0;
    m->refine = 0;
}

// The census says how many cells hold points (m->occ): coarsen the grid so that an occupied cell holds about `target` points
// (surface-like data: points per cell grow with h^2) and, if so, clear the counts for the second count -- one launch: every
// workgroup takes the decision from the same words (n, occ), the first one also writes the new grid (which nobody reads here).
__global__ void __launch_bounds__(GRID_BLK) grid_refine_zero_kernel(GridMeta *__restrict__ m, size_t n, double target, uint32_t *__restrict__ words, size_t nwords) {
    const uint32_t occ = m->occ;
    const double ppc = (double)n / (double)(occ ? occ : 1u);
    if (!(ppc < target)) return;
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < nwords; i += (size_t)gridDim.x * GRID_BLK) words[i] = 0;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double h = m->g.h * sqrt(target / ppc);
    if (h > m->maxext) h = m->maxext;
    Grid g = m->g;
    grid_dims(g, m->ext, h);
    m->g = g;
    m->refine = 1;
}

// ---- bounding box ----
__global__ void __launch_bounds__(GRID_BLK) bbox_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                  float *__restrict__ partial /* [gridDim.x][6] */) {
    __shared__ float red[6][GRID_BLK / 64];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) {
        float v[3] = {x[i], y[i], z[i]};
        if (!(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]))) continue;
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], v[a]); hi[a] = fmaxf(hi[a], v[a]); }
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
        for (int w = 1; w < GRID_BLK / 64; w++) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
        partial[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}

// ---- occupancy probe / counting sort ----
// Consecutive points of a cloud in scan order mostly share a cell: one atomic per RUN of equal cells inside a wave, not per
// point (the scattered atomics of these two kernels were their whole cost: 10 M of them take ~0.4 ms).  `run` describes the
// run a lane belongs to: its first lane and its length.
struct WaveRun { int first; int length; bool leads; };
__device__ __forceinline__ WaveRun wave_run(uint32_t c, bool active) {
    const int lane = threadIdx.x & 63;
    const uint32_t prev = (uint32_t)__shfl_up((int)c, 1, 64);
    const bool leads = active && (lane == 0 || prev != c);
    const unsigned long long L = __ballot(leads), A = __ballot(active);
    WaveRun r;
    r.leads = leads;
    const unsigned long long upto = L & ((2ull << lane) - 1ull);                 // leaders at or below this lane
    r.first = upto ? 63 - __builtin_clzll(upto) : lane;
    const unsigned long long above = r.first < 63 ? (L >> (r.first + 1)) : 0ull;  // the next run's leader, if any
    const int end = above ? r.first + 1 + __builtin_ctzll(above) : (A ? 64 - __builtin_clzll(A) : 0);
    r.length = end - r.first;
    return r;
}

// census: also count the cells that get their first point here (the adds then return what was there), one atomic per workgroup
// on *census -- a separate pass over the whole cell array for it was a launch of its own
__global__ void __launch_bounds__(GRID_BLK) cell_count_kernel(const GridMeta *__restrict__ gm, int second_count, const float *__restrict__ x,
                                                        const float *__restrict__ y, const float *__restrict__ z, size_t n, uint32_t *__restrict__ counts,
                                                        uint32_t *__restrict__ cell_id, uint32_t *__restrict__ census) {
    if (second_count && !gm->refine) return;   // the census's grid stands: its counts do too
    const Grid g = gm->g;
    uint32_t fresh = 0;
    for (size_t base = (size_t)blockIdx.x * GRID_BLK; base < n; base += (size_t)gridDim.x * GRID_BLK) {
        const size_t i = base + threadIdx.x;
        const bool active = i < n;
        uint32_t c = 0xffffffffu;
        if (active) {
            c = cell_of(g, x[i], y[i], z[i]);
            if (cell_id) cell_id[i] = c;
        }
        const WaveRun r = wave_run(c, active);
        if (census) {
            if (r.leads && atomicAdd(&counts[c], (uint32_t)r.length) == 0u) fresh++;
        } else if (r.leads) {
            atomicAdd(&counts[c], (uint32_t)r.length);
        }
    }
    if (!census) return;
    __shared__ uint32_t wsum[GRID_BLK / 64];
    k::wave_reduce_sum(fresh);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = fresh;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < GRID_BLK / 64; w++) t += wsum[w];
        if (t) atomicAdd(census, t);
    }
}

// starts = exclusive prefix sums of counts over the cells of the grid the device decided on (gm->g): ONE workgroup, for the
// small clouds of the dense layout (a camera tile of a frame: a few ten thousand cells).  rocprim's scan runs over the whole
// allocation (the host does not know the grid: 8 cells per point whatever the kernels made of them) in two launches, 9 + 3 us for
// such a tile; this one reads the cell count where the grid is and takes a pass to add and a pass to write.
constexpr int SCAN1_THREADS = 1024, SCAN1_PRE = 12;   // 12 groups of four cells per thread in registers: 48 k cells per round (16: spills)
__device__ __forceinline__ uint32_t scan1_wave_inclusive(uint32_t v) {   // four DPP row shifts inside rows of 16, two row broadcasts across them
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
__global__ void __launch_bounds__(SCAN1_THREADS) small_scan_kernel(const GridMeta *__restrict__ gm, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ counts2,
                                                                  uint32_t *__restrict__ starts, size_t cap) {
    __shared__ uint32_t wsum[2][SCAN1_THREADS / 64];
    const GridSlot slot = grid_slot(gm, counts, counts2);
    size_t ncells = grid_cells(slot.gm->g);
    if (ncells > cap) ncells = cap;
    // Whole 16-byte groups (the arrays are pool blocks, cap is a multiple of four, and what lies between the grid's last cell and the end
    // of its group is zeroes).  A round: up to twelve slices of 1024 groups, lane t of the workgroup taking group t of every slice -- every
    // load and store instruction of a wave covers 1 KB in one piece, and all of a round's loads are in flight before the first is used --
    // then slice by slice: the lanes' sums, a DPP scan over the wave, the waves' totals through LDS (one barrier per slice of 4096 cells).
    // (Versions before this one, all measured on a 35 k-cell grid, where an empty kernel of this shape takes 6 us by events: a contiguous
    // share per thread in two passes 15 us -- 144 bytes per lane apart, every wave instruction sixty-four separate requests on ONE compute
    // unit; tiles of 16 k cells with 64 contiguous bytes per lane 13 us; with that tile's loads under a condition, which the compiler turned
    // into sixteen one-word loads behind a branch each, 25 us.  rocprim's two launches over the whole allocation: 11.6.)
    const size_t nvec = (ncells + 3) / 4, vlast = cap / 4 - 1;
    const uint4 *c4 = reinterpret_cast<const uint4 *>(slot.counts);
    uint4 *s4 = reinterpret_cast<uint4 *>(starts);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint32_t carry = 0, flip = 0;
    for (size_t base = 0; base < nvec; base += (size_t)SCAN1_THREADS * SCAN1_PRE) {
        uint4 q[SCAN1_PRE];
#pragma unroll
        for (int j = 0; j < SCAN1_PRE; j++) {
            const size_t v = base + (size_t)j * SCAN1_THREADS + threadIdx.x;
            q[j] = c4[v < vlast ? v : vlast];   // (the address clamped into the allocation, the VALUE chosen afterwards: no load under a condition)
        }
#pragma unroll
        for (int j = 0; j < SCAN1_PRE; j++) {
            const size_t v = base + (size_t)j * SCAN1_THREADS + threadIdx.x;
            if (base + (size_t)j * SCAN1_THREADS >= nvec) continue;   // (the same for every lane: the barrier below is met by all or none)
            const uint4 w = v < nvec ? q[j] : zero;
            const uint32_t mine = w.x + w.y + w.z + w.w;
            const uint32_t incl = scan1_wave_inclusive(mine);
            uint32_t (&ws)[SCAN1_THREADS / 64] = wsum[flip & 1u];   // (two sets: the next slice's writers do not wait for this slice's readers)
            flip++;
            if (lane == 63) ws[wave] = incl;
            __syncthreads();
            uint32_t before = carry + incl - mine, total = 0;
#pragma unroll
            for (int k = 0; k < SCAN1_THREADS / 64; k++) {
                const uint32_t t = ws[k];
                if (k < wave) before += t;
                total += t;
            }
            carry += total;
            if (v < nvec) s4[v] = make_uint4(before, before + w.x, before + w.x + w.y, before + w.x + w.y + w.z);
        }
    }
}

// ---- small clouds (r4): the dense layout in ten launches instead of twelve ----
// A camera tile of a frame (a few ten thousand points) is filtered in ~0.1 ms, most of it the chain of small kernels in front of
// the search.  Here the box kernel also clears the per-cell arrays (their size is the host's: 8 cells per point), EVERY workgroup of
// the first count derives the grid from the partial boxes itself (a few KB from L2 and one lane's arithmetic: the same grid in every
// workgroup) and the first one writes it down; every workgroup of the second count takes the coarsening decision from the same
// two words and, if it stands, derives the coarser grid itself and counts into an array of its own (cleared with the others), the
// first one writing the grid into the block's second slot.  What follows reads slot 1 if its `refine` says so, slot 0 otherwise.
__device__ __forceinline__ void finest_grid(const float lo[3], const float hi[3], size_t cap_cells, GridMeta &m) {   // grid_setup_zero_kernel's arithmetic
    Grid g;
    double ext[3], maxext = 0;
    for (int a = 0; a < 3; a++) {
        g.mn[a] = lo[a] == FLT_MAX ? 0.f : lo[a];
        ext[a] = (double)hi[a] - (double)lo[a];
        if (!(ext[a] >= 0)) ext[a] = 0;   // no finite point
        if (ext[a] > maxext) maxext = ext[a];
    }
    if (!(maxext > 0)) maxext = 1.0;
    double h = maxext / 1024.0;
    grid_dims(g, ext, h);
    while (grid_cells(g) > cap_cells) { h *= 1.25; grid_dims(g, ext, h); }
    m.g = g;
    for (int a = 0; a < 3; a++) m.ext[a] = ext[a];
    m.maxext = maxext;
}

__global__ void __launch_bounds__(GRID_BLK) small_bbox_zero_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                             float *__restrict__ partial /* [gridDim.x][6] */, uint32_t *__restrict__ words, size_t nwords,
                                                             GridMeta *__restrict__ m) {
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint4 *w4 = reinterpret_cast<uint4 *>(words);
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < nwords / 4; i += (size_t)gridDim.x * GRID_BLK) w4[i] = zero;   // (nwords: a multiple of four)
    if (blockIdx.x == 0 && threadIdx.x < 2) { m[threadIdx.x].occ = 0; m[threadIdx.x].refine = 0; }
    __shared__ float red[6][GRID_BLK / 64];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) {
        float v[3] = {x[i], y[i], z[i]};
        if (!(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]))) continue;
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], v[a]); hi[a] = fmaxf(hi[a], v[a]); }
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
        for (int w = 1; w < GRID_BLK / 64; w++) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
        partial[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}

// PHASE 0: grid from the partial boxes, count + census into counts, slot 0.  PHASE 1: the coarser grid if the census asks for one,
// count into counts2, slot 1.
template <int PHASE>
__global__ void __launch_bounds__(GRID_BLK) small_count_kernel(const float *__restrict__ partial, unsigned nb, size_t cap_cells, double target, GridMeta *__restrict__ m,
                                                         const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                         uint32_t *__restrict__ counts, uint32_t *__restrict__ cell_id) {
    __shared__ GridMeta sm;
    __shared__ uint32_t wsum[GRID_BLK / 64];
    if (PHASE == 0) {
        if (threadIdx.x < 64) {
            float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
            for (unsigned b = threadIdx.x; b < nb; b += 64)
                for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], partial[b * 6 + a]); hi[a] = fmaxf(hi[a], partial[b * 6 + 3 + a]); }
            for (int a = 0; a < 3; a++)
                for (int off = 32; off > 0; off >>= 1) { lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64)); hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64)); }
            if (threadIdx.x == 0) {
                finest_grid(lo, hi, cap_cells, sm);
                if (blockIdx.x == 0) { m[0].g = sm.g; for (int a = 0; a < 3; a++) m[0].ext[a] = sm.ext[a]; m[0].maxext = sm.maxext; }   // (occ: the census's adds, cleared by the box kernel)
            }
        }
    } else {
        const uint32_t occ = m[0].occ;
        const double ppc = (double)n / (double)(occ ? occ : 1u);
        if (!(ppc < target)) return;   // the census's grid stands, and its counts (the whole workgroup leaves: the same words for every thread)
        if (threadIdx.x == 0) {
            double h = m[0].g.h * sqrt(target / ppc);
            if (h > m[0].maxext) h = m[0].maxext;
            Grid g = m[0].g;
            double ext[3] = {m[0].ext[0], m[0].ext[1], m[0].ext[2]};
            grid_dims(g, ext, h);
            sm.g = g;
            if (blockIdx.x == 0) { m[1].g = g; m[1].refine = 1; }
        }
    }
    __syncthreads();
    const Grid g = sm.g;
    uint32_t fresh = 0;
    for (size_t base = (size_t)blockIdx.x * GRID_BLK; base < n; base += (size_t)gridDim.x * GRID_BLK) {
        const size_t i = base + threadIdx.x;
        const bool active = i < n;
        uint32_t c = 0xffffffffu;
        if (active) {
            c = cell_of(g, x[i], y[i], z[i]);
            cell_id[i] = c;
        }
        const WaveRun r = wave_run(c, active);
        if (PHASE == 0) {
            if (r.leads && atomicAdd(&counts[c], (uint32_t)r.length) == 0u) fresh++;
        } else if (r.leads) {
            atomicAdd(&counts[c], (uint32_t)r.length);
        }
    }
    if (PHASE != 0) return;
    k::wave_reduce_sum(fresh);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = fresh;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < GRID_BLK / 64; w++) t += wsum[w];
        if (t) atomicAdd(&m[0].occ, t);
    }
}

// sorted[pos] = (x, y, z, original index)
__global__ void __launch_bounds__(GRID_BLK) cell_scatter_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                          const uint32_t *__restrict__ cell_id, const uint32_t *__restrict__ cell_start,
                                                          uint32_t *__restrict__ cell_fill, float4 *__restrict__ sorted) {
    for (size_t base = (size_t)blockIdx.x * GRID_BLK; base < n; base += (size_t)gridDim.x * GRID_BLK) {
        const size_t i = base + threadIdx.x;
        const bool active = i < n;
        const uint32_t c = active ? cell_id[i] : 0xffffffffu;
        const WaveRun r = wave_run(c, active);
        // the run's leader reserves room for the whole run; the order of points inside a cell does not matter to the search
        uint32_t at = 0;
        if (r.leads) at = cell_start[c] + atomicAdd(&cell_fill[c], (uint32_t)r.length);
        at = (uint32_t)__shfl((int)at, r.first, 64);
        if (active) sorted[at + (uint32_t)((threadIdx.x & 63) - r.first)] = make_float4(x[i], y[i], z[i], __uint_as_float((uint32_t)i));
    }
}

// ---- sparse layout: which segments exist, their cells ----
// id of a point's cell before the segments are numbered: segment << 4 | cell inside the segment
__device__ __forceinline__ uint32_t seg_cell_of(const Grid &g, float x, float y, float z) {
    const uint32_t cx = (uint32_t)cell_coord(g, x, 0);
    const uint32_t seg = (cx >> SEG_SHIFT) + (uint32_t)g.nsegx * ((uint32_t)cell_coord(g, y, 1) + (uint32_t)g.dim[1] * (uint32_t)cell_coord(g, z, 2));
    return (seg << SEG_SHIFT) | (cx & (SEG - 1));
}

// masks[segment] |= bit of the cell; cell_id[i] = seg_cell_of(point i)
__global__ void __launch_bounds__(GRID_BLK) seg_mark_kernel(Grid g, const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                      uint32_t *__restrict__ masks, uint32_t *__restrict__ cell_id) {
    for (size_t base = (size_t)blockIdx.x * GRID_BLK; base < n; base += (size_t)gridDim.x * GRID_BLK) {
        const size_t i = base + threadIdx.x;
        const bool active = i < n;
        uint32_t c = 0xffffffffu;
        if (active) {
            c = seg_cell_of(g, x[i], y[i], z[i]);
            cell_id[i] = c;
        }
        const WaveRun r = wave_run(c, active);
        if (r.leads) atomicOr(&masks[c >> SEG_SHIFT], 1u << (c & (SEG - 1)));
    }
}

// flags[s] = segment s holds points; out[0] += occupied cells, out[1] += occupied segments (one atomic pair per workgroup)
__global__ void __launch_bounds__(GRID_BLK) seg_census_kernel(const uint32_t *__restrict__ masks, size_t nseg, uint32_t *__restrict__ flags, uint32_t *__restrict__ out) {
    __shared__ uint32_t wsum[2][GRID_BLK / 64];
    uint32_t cells = 0, segs = 0;
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < nseg; i += (size_t)gridDim.x * GRID_BLK) {
        const uint32_t m = masks[i];
        flags[i] = m != 0u;
        cells += (uint32_t)__popc(m);
        segs += m != 0u;
    }
    for (int off = 32; off > 0; off >>= 1) { cells += __shfl_down(cells, off, 64); segs += __shfl_down(segs, off, 64); }   // (two sums a step)
    if ((threadIdx.x & 63) == 0) { wsum[0][threadIdx.x >> 6] = cells; wsum[1][threadIdx.x >> 6] = segs; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
        for (int w = 0; w < GRID_BLK / 64; w++) { a += wsum[0][w]; b += wsum[1][w]; }
        if (a) atomicAdd(&out[0], a);
        if (b) atomicAdd(&out[1], b);
    }
}

// info[s] = (number of occupied segments before s) << 1 | (s is occupied): for an empty segment the first half names the
// next occupied one, which is what a range lookup wants from it
__global__ void __launch_bounds__(GRID_BLK) seg_pack_kernel(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ before, size_t nseg, uint32_t *__restrict__ info) {
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < nseg; i += (size_t)gridDim.x * GRID_BLK) info[i] = (before[i] << 1) | flags[i];
}

// cell_id[i]: seg_cell_of -> number of the cell among the cells that exist; counts[cell]++ (one atomic per run, as above)
__global__ void __launch_bounds__(GRID_BLK) seg_count_kernel(const uint32_t *__restrict__ info, size_t n, uint32_t *__restrict__ cell_id, uint32_t *__restrict__ counts) {
    for (size_t base = (size_t)blockIdx.x * GRID_BLK; base < n; base += (size_t)gridDim.x * GRID_BLK) {
        const size_t i = base + threadIdx.x;
        const bool active = i < n;
        uint32_t c = 0xffffffffu;
        if (active) {
            const uint32_t sc = cell_id[i];
            c = ((info[sc >> SEG_SHIFT] >> 1) << SEG_SHIFT) | (sc & (SEG - 1));
            cell_id[i] = c;
        }
        const WaveRun r = wave_run(c, active);
        if (r.leads) atomicAdd(&counts[c], (uint32_t)r.length);
    }
}

// Tuning knobs: cells per point that a dense grid may have at most, and the points an occupied cell should hold, as a fraction of
// k + 1 (`fraction` when CWIPC_SOR_CELL_TARGET is not set)
size_t sor_cells_per_point() {
    static const size_t cpp = []() { const char *e = getenv("CWIPC_SOR_CELLS_PER_POINT"); return e && atoi(e) > 0 ? (size_t)atoi(e) : (size_t)8; }();
    return cpp;
}
double sor_cell_target(int k, double fraction) {
    static const double knob = []() { const char *e = getenv("CWIPC_SOR_CELL_TARGET"); return e ? atof(e) : NAN; }();
    return (double)(k + 1) * (std::isnan(knob) ? fraction : knob);
}

// The dense layout, driven from the device: box -> grid -> census -> (coarser grid, second count) -> counting sort -> search,
// sixteen launches and no wait (the caller has one further down, behind the compaction).  Arrays are sized for the largest
// grid the rules allow (a few cells per point), whatever the kernels then decide.
bool sor_dense_on_device(const DeviceSoA &src, int k, float *partial, unsigned nb, ThreadCtx &c, const GridSearch &search) {
    const size_t n = src.npoints;
    const size_t cap = std::min<size_t>(MAX_CELLS, std::max<size_t>((size_t)1 << 16, sor_cells_per_point() * n));
    const double target = sor_cell_target(k, 0.5);
    GridMeta *meta = (GridMeta *)pool_alloc(sizeof(GridMeta));
    uint32_t *counts = (uint32_t *)pool_alloc(cap * sizeof(uint32_t));
    uint32_t *starts = (uint32_t *)pool_alloc(cap * sizeof(uint32_t));
    uint32_t *cursor = (uint32_t *)pool_alloc(cap * sizeof(uint32_t));
    uint32_t *cell_id = (uint32_t *)pool_alloc(n * sizeof(uint32_t));
    float4 *sorted = (float4 *)pool_alloc(n * sizeof(float4));
    void *scan_tmp = nullptr;
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_bytes, counts, starts, 0u, cap, rocprim::plus<uint32_t>(), c.stream);
    if (e == hipSuccess) scan_tmp = pool_alloc(tmp_bytes ? tmp_bytes : 256);
    auto give_back = [&](bool later) {
        void *all[] = {partial, meta, counts, starts, cursor, cell_id, sorted, scan_tmp};
        for (void *b : all) { if (later) c.free_later(b); else pool_free(b); }
    };
    if (e != hipSuccess || !meta || !counts || !starts || !cursor || !cell_id || !sorted || !scan_tmp) {
        (void)c.sync();
        give_back(false);
        return hip_failed(e != hipSuccess ? e : hipErrorOutOfMemory, "sor workspace", __FILE__, __LINE__);
    }
    const Grid unused{};
    const unsigned cap_grid = std::min(1024u, grid_blocks(cap / 4 + 1));
    // (round 3: eleven launches instead of seventeen -- the two memsets ride with the grid's set-up, the census with the first
    // count, the coarsening with the clearing it asks for; a camera tile's kernels cost the device less than their launches
    // cost the host)
    CW_LAUNCH("sor_grid_setup", grid_setup_zero_kernel, dim3(cap_grid), dim3(GRID_BLK), 0, c.stream, partial, nb, cap, meta, counts, cursor);
    bool ok = true;
    if (ok) {
        CW_LAUNCH("sor_cell_count", cell_count_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, meta, 0, src.x(), src.y(), src.z(), n, counts, cell_id, &meta->occ);
        CW_LAUNCH("sor_grid_refine", grid_refine_zero_kernel, dim3(cap_grid), dim3(GRID_BLK), 0, c.stream, meta, n, target, counts, cap);
        CW_LAUNCH("sor_cell_count", cell_count_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, meta, 1, src.x(), src.y(), src.z(), n, counts, cell_id, (uint32_t *)nullptr);
        if (profiling_enabled()) profile_begin("sor_exclusive_scan", c.stream);
        e = rocprim::exclusive_scan(scan_tmp, tmp_bytes, counts, starts, 0u, cap, rocprim::plus<uint32_t>(), c.stream);
        if (profiling_enabled()) profile_end(c.stream);
        ok = e == hipSuccess;
    }
    if (ok) {
        CW_LAUNCH("sor_cell_scatter", cell_scatter_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, src.x(), src.y(), src.z(), n, cell_id, starts, cursor,
                  sorted);
        ok = search(GridView{unused, meta, sorted, n, starts, counts, nullptr, false}, c.stream);
    }
    ok = hipGetLastError() == hipSuccess && ok;
    if (!ok) {
        hip_failed(e != hipSuccess ? e : hipGetLastError(), "sor k-NN", __FILE__, __LINE__);
        (void)c.sync();
        give_back(false);
        return false;
    }
    give_back(true);
    return true;
}

// The same for small clouds (cap <= 2^19 cells: up to 64 k points; a search that reads all layouts): ten launches with the compaction behind it, see small_bbox_zero_kernel.
bool sor_small_on_device(const DeviceSoA &src, int k, size_t cap, ThreadCtx &c, const GridSearch &search) {
    const size_t n = src.npoints;
    const double target = sor_cell_target(k, 0.5);
    const unsigned nb = std::min(256u, grid_blocks(n));
    float *partial = (float *)pool_alloc((size_t)nb * 6 * sizeof(float));
    GridMeta *meta = (GridMeta *)pool_alloc(2 * sizeof(GridMeta));
    uint32_t *words = (uint32_t *)pool_alloc(3 * cap * sizeof(uint32_t));   // counts | counts of the coarser grid | the scatter's cursor
    uint32_t *starts = (uint32_t *)pool_alloc(cap * sizeof(uint32_t));
    uint32_t *cell_id = (uint32_t *)pool_alloc(n * sizeof(uint32_t));
    float4 *sorted = (float4 *)pool_alloc(n * sizeof(float4));
    auto give_back = [&](bool later) {
        void *all[] = {partial, meta, words, starts, cell_id, sorted};
        for (void *b : all) { if (later) c.free_later(b); else pool_free(b); }
    };
    if (!partial || !meta || !words || !starts || !cell_id || !sorted) {
        (void)c.sync();
        give_back(false);
        return hip_failed(hipErrorOutOfMemory, "sor workspace", __FILE__, __LINE__);
    }
    uint32_t *counts = words, *counts2 = words + cap, *cursor = words + 2 * cap;
    const Grid unused{};
    const unsigned pgrid = grid_blocks(n);
    CW_LAUNCH("sor_bbox", small_bbox_zero_kernel, dim3(nb), dim3(GRID_BLK), 0, c.stream, src.x(), src.y(), src.z(), n, partial, words, 3 * cap, meta);
    CW_LAUNCH("sor_cell_count", small_count_kernel<0>, dim3(pgrid), dim3(GRID_BLK), 0, c.stream, partial, nb, cap, target, meta, src.x(), src.y(), src.z(), n, counts, cell_id);
    CW_LAUNCH("sor_cell_count", small_count_kernel<1>, dim3(pgrid), dim3(GRID_BLK), 0, c.stream, partial, nb, cap, target, meta, src.x(), src.y(), src.z(), n, counts2, cell_id);
    CW_LAUNCH("sor_exclusive_scan", small_scan_kernel, dim3(1), dim3(SCAN1_THREADS), 0, c.stream, meta, counts, counts2, starts, cap);
    CW_LAUNCH("sor_cell_scatter", cell_scatter_kernel, dim3(pgrid), dim3(GRID_BLK), 0, c.stream, src.x(), src.y(), src.z(), n, cell_id, starts, cursor, sorted);
    const bool searched = search(GridView{unused, meta, sorted, n, starts, counts, counts2, false}, c.stream);
    if (hipGetLastError() != hipSuccess || !searched) {
        hip_failed(hipGetLastError(), "sor k-NN", __FILE__, __LINE__);
        (void)c.sync();
        give_back(false);
        return false;
    }
    give_back(true);
    return true;
}

}  // namespace

bool grid_and_search(const DeviceSoA &src, int k, bool all_layouts, const GridSearch &search) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t n = src.npoints;
    if (n == 0) return true;

    static const int sparse_knob = []() { const char *e = getenv("CWIPC_SOR_SPARSE"); return e ? atoi(e) : -1; }();   // test knob: 1 always, 0 never
    const bool sparse = (sparse_knob == 1 || (sparse_knob != 0 && n >= ((size_t)1 << 20))) && all_layouts;
    if (!sparse && all_layouts) {
        // (r4) small clouds: two launches fewer and a one-workgroup scan over the cells the grid really has
        static const size_t small_cells = []() { const char *e = getenv("CWIPC_SOR_SMALL_CELLS"); return e ? (size_t)atol(e) : (size_t)1 << 19; }();   // 0: never (test knob)
        const size_t cap = std::min<size_t>(MAX_CELLS, std::max<size_t>((size_t)1 << 16, sor_cells_per_point() * n));
        if (cap <= small_cells) return sor_small_on_device(src, k, cap, c, search);
    }
    // bounding box (the dense layout reads it on the device, the sparse one on the host)
    const unsigned nb = grid_blocks(n);
    float *partial = (float *)pool_alloc((size_t)nb * 6 * sizeof(float));
    if (!partial) return false;
    CW_LAUNCH("sor_bbox", bbox_kernel, dim3(nb), dim3(GRID_BLK), 0, c.stream, src.x(), src.y(), src.z(), n, partial);
    if (!sparse) return sor_dense_on_device(src, k, partial, nb, c, search);
    // ---- big clouds: the sparse layout (segments of 16 cells, only those that hold points), on the box the host has read back ----
    float *hpart = (float *)c.staging((size_t)nb * 6 * sizeof(float));
    bool ok = hpart && hipMemcpyAsync(hpart, partial, (size_t)nb * 6 * sizeof(float), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(partial);
    if (!ok) return false;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (unsigned b = 0; b < nb; b++)
        for (int a = 0; a < 3; a++) {
            mn[a] = fminf(mn[a], hpart[b * 6 + a]);
            mx[a] = fmaxf(mx[a], hpart[b * 6 + 3 + a]);
        }
    double ext[3], maxext = 0;
    for (int a = 0; a < 3; a++) {
        ext[a] = (double)mx[a] - (double)mn[a];
        if (!(ext[a] >= 0)) ext[a] = 0;   // no finite point
        if (ext[a] > maxext) maxext = ext[a];
    }
    if (!(maxext > 0)) maxext = 1.0;

    auto make_grid = [&](double h) {
        Grid g;
        for (int a = 0; a < 3; a++) {
            g.mn[a] = mn[a] == FLT_MAX ? 0.f : mn[a];
            g.dim[a] = (int)floor(ext[a] / h) + 1;
        }
        g.h = h;
        g.inv_h = 1.0 / h;
        g.nsegx = (g.dim[0] + SEG - 1) / SEG;
        return g;
    };
    auto cells_of = [](const Grid &g) { return (size_t)g.dim[0] * (size_t)g.dim[1] * (size_t)g.dim[2]; };
    static const size_t sparse_cpp = []() { const char *e = getenv("CWIPC_SOR_SPARSE_CELLS_PER_POINT"); return e && atoi(e) > 0 ? (size_t)atoi(e) : (size_t)16; }();
    // cells of the (virtual) fine grid: a few dozen per point, and segment numbers must fit 27 bits
    const size_t budget = std::min<size_t>((size_t)1 << 30, std::max<size_t>((size_t)1 << 16, sparse_cpp * n));
    auto segs_of = [](const Grid &gg) { return (size_t)gg.nsegx * (size_t)gg.dim[1] * (size_t)gg.dim[2]; };
    double hs = maxext / 2048.0;
    while (cells_of(make_grid(hs)) > budget || segs_of(make_grid(hs)) >= ((size_t)1 << 27)) hs *= 1.25;
    Grid g = make_grid(hs);
    size_t nseg = segs_of(g);
    uint32_t *cell_id = (uint32_t *)pool_alloc(n * sizeof(uint32_t));
    float4 *sorted = (float4 *)pool_alloc(n * sizeof(float4));
    uint32_t *masks = nullptr, *flags = nullptr, *before = nullptr, *info = nullptr, *counts = nullptr, *starts = nullptr, *cursor = nullptr;
    void *scan_tmp = nullptr;
    auto give_back = [&](bool later) {
        void *all[] = {cell_id, sorted, masks, flags, before, info, counts, starts, cursor, scan_tmp};
        for (void *b : all) { if (later) c.free_later(b); else pool_free(b); }
    };
    auto fail = [&]() { (void)c.sync(); give_back(false); return false; };
    if (!cell_id || !sorted) return fail();
    uint32_t occ_cells = 0, occ_segs = 0;
    auto census = [&]() -> bool {
        pool_free(masks); pool_free(flags);
        masks = (uint32_t *)pool_alloc(nseg * sizeof(uint32_t) + 256);
        flags = (uint32_t *)pool_alloc(nseg * sizeof(uint32_t));
        if (!masks || !flags) return false;
        uint32_t *out = masks + nseg;
        bool good = hipMemsetAsync(masks, 0, nseg * sizeof(uint32_t) + 8, c.stream) == hipSuccess;
        if (!good) return false;
        CW_LAUNCH("sor_seg_mark", seg_mark_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, g, src.x(), src.y(), src.z(), n, masks, cell_id);
        CW_LAUNCH("sor_seg_census", seg_census_kernel, dim3(std::min(1024u, grid_blocks(nseg))), dim3(GRID_BLK), 0, c.stream, masks, nseg, flags, out);
        good = hipMemcpyAsync(c.host_words, out, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        good = c.sync() && good;
        occ_cells = c.host_words[0];
        occ_segs = c.host_words[1];
        return good;
    };
    if (!census()) return fail();
    {
        // coarsen so that an occupied cell holds about 0.3 (k + 1) points (surface-like data: points per cell grow with h^2).
        // (r4: 0.5 (k + 1) until the shells beyond the first got their bound per row; with it finer cells pay: 2 M points 0.71 -> 0.66 ms,
        // profiles/r04_sor_small_flow.txt.  10 M points are at the segment budget's cell size either way.)
        const double ppc = (double)n / (double)(occ_cells ? occ_cells : 1);
        const double target = sor_cell_target(k, 0.3);
        if (ppc < target) {
            double h = hs * sqrt(target / ppc);
            if (h > maxext) h = maxext;
            g = make_grid(h);
            nseg = segs_of(g);
            if (!census()) return fail();
        }
    }
    const size_t ncomp = (size_t)occ_segs << SEG_SHIFT;
    before = (uint32_t *)pool_alloc(nseg * sizeof(uint32_t));
    info = (uint32_t *)pool_alloc(nseg * sizeof(uint32_t));
    counts = (uint32_t *)pool_alloc((ncomp + 1) * sizeof(uint32_t));
    starts = (uint32_t *)pool_alloc((ncomp + 1) * sizeof(uint32_t));
    cursor = (uint32_t *)pool_alloc((ncomp + 1) * sizeof(uint32_t));
    if (!before || !info || !counts || !starts || !cursor) return fail();
    size_t tmp_a = 0, tmp_b = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_a, flags, before, 0u, nseg, rocprim::plus<uint32_t>(), c.stream);
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_b, counts, starts, 0u, ncomp + 1, rocprim::plus<uint32_t>(), c.stream);
    const size_t tmp_bytes = std::max(tmp_a, tmp_b);
    if (e == hipSuccess) {
        scan_tmp = pool_alloc(tmp_bytes ? tmp_bytes : 256);
        if (!scan_tmp) e = hipErrorOutOfMemory;
    }
    if (e != hipSuccess) { hip_failed(e, "rocprim::exclusive_scan", __FILE__, __LINE__); return fail(); }
    if (profiling_enabled()) profile_begin("sor_exclusive_scan", c.stream);
    e = rocprim::exclusive_scan(scan_tmp, tmp_a, flags, before, 0u, nseg, rocprim::plus<uint32_t>(), c.stream);
    if (profiling_enabled()) profile_end(c.stream);
    ok = e == hipSuccess;
    if (ok) CW_LAUNCH("sor_seg_pack", seg_pack_kernel, dim3(std::min(2048u, grid_blocks(nseg))), dim3(GRID_BLK), 0, c.stream, flags, before, nseg, info);
    ok = ok && hipMemsetAsync(counts, 0, (ncomp + 1) * sizeof(uint32_t), c.stream) == hipSuccess &&
         hipMemsetAsync(cursor, 0, (ncomp + 1) * sizeof(uint32_t), c.stream) == hipSuccess;
    if (ok) {
        CW_LAUNCH("sor_cell_count", seg_count_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, info, n, cell_id, counts);
        if (profiling_enabled()) profile_begin("sor_exclusive_scan", c.stream);
        e = rocprim::exclusive_scan(scan_tmp, tmp_b, counts, starts, 0u, ncomp + 1, rocprim::plus<uint32_t>(), c.stream);
        if (profiling_enabled()) profile_end(c.stream);
        ok = e == hipSuccess;
    }
    if (ok) {
        CW_LAUNCH("sor_cell_scatter", cell_scatter_kernel, dim3(grid_blocks(n)), dim3(GRID_BLK), 0, c.stream, src.x(), src.y(), src.z(), n, cell_id, starts,
                  cursor, sorted);
        ok = search(GridView{g, nullptr, sorted, n, starts, info, nullptr, true}, c.stream);
    }
    ok = hipGetLastError() == hipSuccess && ok;
    if (!ok) { hip_failed(e != hipSuccess ? e : hipGetLastError(), "sor k-NN (sparse grid)", __FILE__, __LINE__); return fail(); }
    give_back(true);   // (no wait here: every caller has one further down, and the temporaries go back to the pool there)
    return true;
}

}  // namespace cwipc_amd
