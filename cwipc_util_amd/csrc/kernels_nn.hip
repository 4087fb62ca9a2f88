// kernels_nn.hip -- nearest distances from one cloud to another on gfx950 (the registration analyzer).
//
// Reference: python/cwipc/registration/analyze.py:120-123, scipy.spatial.KDTree.query(points, k=[nth + 1], distance_upper_bound=max):
// per SOURCE point the distance to its (nth + 1)-th nearest REFERENCE point, inf when fewer than nth + 1 lie closer than max.
// Here the squared distance, in f64: d2 = (dx*dx + dy*dy) + dz*dz with dx = (double)qx - (double)px, every operation rounded on
// its own (-ffp-contract=off) -- what scipy's tree holds before its final sqrt, bit for bit; the caller takes the root on the host.
//
// The grid is the point grid built over the reference cloud (grid_and_search, any of its three flows); the queries are the
// points of another cloud, one lane each, in the caller's order, wherever they lie:
//   * the search starts from the query's cell CLAMPED to the grid and is the exact walk of exact_walk.hpp (walk_exact: the shells,
//     the short f64 bounds, the stop rule -- stated there, once, for this file's two kernels and the ICP correspondences), with
//     the (nth + 1)-th candidate so far and max_distance as its limit.  A query far from every reference point with no
//     max_distance therefore scans the whole grid: correct, and as slow as it sounds;
//   * the candidate list is kept in f64 (KCAP = 2, 4 or 32 sorted registers), so the selection is made on the very values that are
//     returned -- an fp32 search with a margin and a second pass would read every candidate's coordinates twice to save registers
//     that this kernel has to spare (at the tooling's nth of 0 or 1 the list is two registers pairs).
// A distance is a value: which of two equally distant points is kept, and the order the counting sort left a cell's points in,
// cannot change it -- two calls give the same bits.
#include "point_grid.hpp"

#include <algorithm>
#include <cstring>

namespace cwipc_amd {

namespace {

constexpr int NN_GRID_WIDTH = 15;

struct NNArgs {
    const float *qx, *qy, *qz;   // the source cloud's planes
    size_t nq;
    int want;                    // nth + 1
    double max2;                 // max_distance^2 in f64 (inf: no bound); candidates must be strictly below
    double *out;                 // nq squared distances, the caller's order
};

__global__ void __launch_bounds__(GRID_BLK) nn_fill_inf_kernel(double *__restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK) out[i] = INFINITY;
}

template <int KCAP, bool SPARSE>
__global__ void __launch_bounds__(QB) nn_distance2_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted,
                                                         const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_count,
                                                         const uint32_t *__restrict__ cell_count2, NNArgs A) {
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    if (qi >= A.nq) return;
    const float qf[3] = {A.qx[qi], A.qy[qi], A.qz[qi]};
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    const int c[3] = {cell_coord(g, qf[0], 0), cell_coord(g, qf[1], 1), cell_coord(g, qf[2], 2)};
    const int pad = KCAP - A.want;
    double best[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; j++) best[j] = j < pad ? -INFINITY : INFINITY;
    // what a candidate has to stay under: the (nth + 1)-th distance so far and the caller's bound
    auto limit = [&]() { return fmin(best[KCAP - 1], A.max2); };
    auto candidate = [&](const float4 p) {
        const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < limit()) {
            // sorted insert, the largest drops out; top down, every slot from old values
#pragma unroll
            for (int j = KCAP - 1; j >= 1; j--) best[j] = d2 < best[j - 1] ? best[j - 1] : fmin(best[j], d2);
            best[0] = fmin(best[0], d2);
        }
    };
    auto scan = [&](uint32_t first, uint32_t last) { scan_range<1>(sorted, first, last, candidate); };
    if constexpr (KCAP > 4) {
        // The list of 32: the scan stays a function call and the list lives in scratch, as the compiler has always built this
        // instantiation (profiles/grid_split_resources.txt, icp_nn_refactor_resources.txt): four or five waves per SIMD.  Inlined
        // into the walk it takes 200 VGPRs, two waves, no scratch -- which of the two is faster has not been timed.
        auto scan_call = [&](uint32_t first, uint32_t last) __attribute__((noinline)) { scan(first, last); };
        walk_exact(rows, q, c, limit, scan_call);
    } else {
        walk_exact(rows, q, c, limit, scan);
    }
    A.out[qi] = best[KCAP - 1];
}

template <int KCAP>
void launch_nn(const GridView &v, const NNArgs &A, hipStream_t s) {
    const unsigned qgrid = (unsigned)((A.nq + QB - 1) / QB);
    if (v.sparse)
        CW_LAUNCH("nn_distance2", (nn_distance2_kernel<KCAP, true>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.starts, v.counts, v.counts2, A);
    else
        CW_LAUNCH("nn_distance2", (nn_distance2_kernel<KCAP, false>), dim3(qgrid), dim3(QB), 0, s, v.g, v.gm, v.sorted, v.starts, v.counts, v.counts2, A);
}

// ---------------------------------------------------------------------------
// The same search for a table of JOBS over one pair of clouds (registration/multicamera.py: every camera of a frame against the
// others, against itself, against a ground truth -- 2N searches whose clouds are all subsets of the same frame).  A job names its
// subsets by predicates -- a tile mask and an open y interval per side -- instead of by compacted clouds: ONE grid over the whole
// reference cloud serves all jobs, the job index is the launch's second grid dimension, and a reference point that takes no part in
// a job is passed over where the scan meets it.  A distance is a value (above), so a job's row holds the very bits that
// nn_distance2 gives for the compacted clouds, whatever grid either of them walked.
//   * the job table lives in device memory (one pool block, copied once per call), in the order of the list widths, so that the
//     jobs of one width are one launch; `row` is the job's place in the caller's list;
//   * a candidate's tile is read from a byte array in SORTED order, written once per call behind the counting sort
//     (nn_gather_tiles_kernel): the scan loads it beside sorted[e], no dependent load through sorted[e].w into rgbt.  Its y is in
//     the register already.  (This layout has not been timed against the dependent load.)
//   * a query that takes no part writes NaN and returns before it touches the grid: the tile word is its first and, when the mask
//     turns it away, its only load;
//   * a job without a participating reference point would send every query through the whole grid (nothing ever bounds its
//     shells): the participants are counted per job first, and such a job's rows are filled (+inf / NaN) instead of searched; so
//     is a job without a participating source point (all NaN).
// ---------------------------------------------------------------------------
struct NNJobDev {
    double max2;             // max_distance^2
    double src_y[2];         // a source point takes part iff src_y[0] < (double)y < src_y[1]
    double ref_y[2];         // the same for reference points
    uint32_t row;            // the job's index in the caller's list: its row of the output
    int32_t want;            // nth + 1
    uint32_t src_mask;       // ... and iff (tile & mask) != 0; 0: every tile
    uint32_t ref_mask;
};

struct NNJobsArgs {
    const float *qx, *qy, *qz;   // the source cloud's planes
    const uint32_t *qrgbt;       // its colour / tile words
    size_t nq;
    const NNJobDev *jobs;        // the first job of this launch (blockIdx.y counts from it)
    double *out;                 // rows of nq squared distances
};

__device__ __forceinline__ bool nn_takes_part(uint32_t tile, float y, uint32_t mask, const double (&lim)[2]) {
    return (mask == 0u || (tile & mask) != 0u) && lim[0] < (double)y && (double)y < lim[1];
}

// tiles[e] = the tile of sorted[e]'s point
__global__ void __launch_bounds__(GRID_BLK) nn_gather_tiles_kernel(const float4 *__restrict__ sorted, const uint32_t *__restrict__ rgbt, size_t n, size_t nref,
                                                                   uint8_t *__restrict__ tiles) {
    for (size_t e = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; e < n; e += (size_t)gridDim.x * GRID_BLK) {
        const uint32_t id = __float_as_uint(sorted[e].w);
        tiles[e] = id < nref ? (uint8_t)(rgbt[id] >> 24) : (uint8_t)0;
    }
}

// counts[2 * (jobs + blockIdx.y) + side] += the points of one cloud that take part in the job as its source (side 0) or reference (1)
__global__ void __launch_bounds__(GRID_BLK) nn_jobs_count_kernel(const float *__restrict__ y, const uint32_t *__restrict__ rgbt, size_t n,
                                                                 const NNJobDev *__restrict__ jobs, int side, uint32_t *__restrict__ counts) {
    const NNJobDev &J = jobs[blockIdx.y];
    const uint32_t mask = side ? J.ref_mask : J.src_mask;
    const double lim[2] = {side ? J.ref_y[0] : J.src_y[0], side ? J.ref_y[1] : J.src_y[1]};
    uint32_t mine = 0;
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * GRID_BLK)
        mine += nn_takes_part(rgbt[i] >> 24, y[i], mask, lim) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&counts[2 * blockIdx.y + side], mine);
}

// the rows of jobs that are not searched: +inf for a query that takes part, NaN for one that does not
__global__ void __launch_bounds__(GRID_BLK) nn_jobs_fill_kernel(NNJobsArgs A) {
    const NNJobDev &J = A.jobs[blockIdx.y];
    double *row = A.out + (size_t)J.row * A.nq;
    for (size_t i = (size_t)blockIdx.x * GRID_BLK + threadIdx.x; i < A.nq; i += (size_t)gridDim.x * GRID_BLK)
        row[i] = nn_takes_part(A.qrgbt[i] >> 24, A.qy[i], J.src_mask, J.src_y) ? (double)INFINITY : (double)NAN;
}

template <int KCAP, bool SPARSE>
__global__ void __launch_bounds__(QB) nn_jobs_kernel(Grid gv, const GridMeta *__restrict__ gm, const float4 *__restrict__ sorted,
                                                    const uint8_t *__restrict__ tiles, const uint32_t *__restrict__ cell_start,
                                                    const uint32_t *__restrict__ cell_count, const uint32_t *__restrict__ cell_count2, NNJobsArgs A) {
    const size_t qi = (size_t)blockIdx.x * QB + threadIdx.x;
    if (qi >= A.nq) return;
    const NNJobDev &J = A.jobs[blockIdx.y];   // (the same for the whole workgroup: scalar loads)
    double *out = A.out + (size_t)J.row * A.nq + qi;
    // a query that takes no part: nothing of the grid is read, and a mask that turns it away has cost this one load
    const uint32_t qtile = A.qrgbt[qi] >> 24;
    if (J.src_mask != 0u && (qtile & J.src_mask) == 0u) { *out = (double)NAN; return; }
    const float qyf = A.qy[qi];
    if (!(J.src_y[0] < (double)qyf && (double)qyf < J.src_y[1])) { *out = (double)NAN; return; }
    const GridRows<SPARSE> rows(gv, gm, cell_start, cell_count, cell_count2);
    const Grid &g = rows.g;
    const float qf[3] = {A.qx[qi], qyf, A.qz[qi]};
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    const int c[3] = {cell_coord(g, qf[0], 0), cell_coord(g, qf[1], 1), cell_coord(g, qf[2], 2)};
    const uint32_t ref_mask = J.ref_mask;
    const double ref_y[2] = {J.ref_y[0], J.ref_y[1]};
    const double max2 = J.max2;
    const int pad = KCAP - J.want;
    double best[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; j++) best[j] = j < pad ? -INFINITY : INFINITY;
    auto limit = [&]() { return fmin(best[KCAP - 1], max2); };
    auto candidate = [&](const float4 p, uint32_t tile) {
        const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        // A reference point that takes no part in this job changes nothing: neither the list nor, through limit(), any bound.  The
        // bounds below therefore only ever depend on accepted candidates, and the walk ends as nn_distance2_kernel's does: when
        // the bound has passed the (nth + 1)-th ACCEPTED candidate or max_distance, or the shells have covered the grid.
        if (nn_takes_part(tile, p.y, ref_mask, ref_y) && d2 < limit()) {
#pragma unroll
            for (int j = KCAP - 1; j >= 1; j--) best[j] = d2 < best[j - 1] ? best[j - 1] : fmin(best[j], d2);
            best[0] = fmin(best[0], d2);
        }
    };
    // sorted[first, last) with the tile bytes beside it, four loads of each in flight (scan_range's shape)
    auto scan = [&](uint32_t first, uint32_t last) {
        uint32_t e = first;
        for (; e + 4 <= last; e += 4) {
            const float4 p0 = sorted[e], p1 = sorted[e + 1], p2 = sorted[e + 2], p3 = sorted[e + 3];
            const uint32_t t0 = tiles[e], t1 = tiles[e + 1], t2 = tiles[e + 2], t3 = tiles[e + 3];
            candidate(p0, t0); candidate(p1, t1); candidate(p2, t2); candidate(p3, t3);
        }
        for (; e < last; e++) candidate(sorted[e], tiles[e]);
    };
    walk_exact(rows, q, c, limit, scan);
    *out = best[KCAP - 1];
}

template <int KCAP>
void launch_nn_jobs(const GridView &v, const uint8_t *tiles, const NNJobsArgs &A, unsigned njobs, hipStream_t s) {
    const dim3 grid((unsigned)((A.nq + QB - 1) / QB), njobs);
    if (v.sparse)
        CW_LAUNCH("nn_jobs", (nn_jobs_kernel<KCAP, true>), grid, dim3(QB), 0, s, v.g, v.gm, v.sorted, tiles, v.starts, v.counts, v.counts2, A);
    else
        CW_LAUNCH("nn_jobs", (nn_jobs_kernel<KCAP, false>), grid, dim3(QB), 0, s, v.g, v.gm, v.sorted, tiles, v.starts, v.counts, v.counts2, A);
}

int nn_width_class(int want) { return want <= 2 ? 0 : want <= 4 ? 1 : 2; }

}  // namespace

size_t nn_jobs_table_bytes(int njobs) { return (size_t)(njobs > 0 ? njobs : 0) * (sizeof(NNJobDev) + 2 * sizeof(uint32_t)); }

bool nn_distance2_jobs(const DeviceSoA &source, const DeviceSoA &reference, const cwipc_hip_nn_job *jobs, int njobs, double *dev_out, void *dev_table) {
    const char *who = "cwipc_hip_nn_distance2_jobs";
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (jobs == nullptr || njobs < 1 || njobs > NN_MAX_JOBS) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "between 1 and 64 jobs");
        return false;
    }
    int maxwant = 1;
    for (int j = 0; j < njobs; j++) {
        const cwipc_hip_nn_job &b = jobs[j];
        if (b.nth < 0 || b.nth > NN_MAX_NTH || !(b.max_distance > 0.0) || std::isnan(b.source_y[0]) || std::isnan(b.source_y[1]) ||
            std::isnan(b.reference_y[0]) || std::isnan(b.reference_y[1])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "nth must lie between 0 and 31, max_distance must be positive (inf: no bound), a y limit is not NaN");
            return false;
        }
        maxwant = std::max(maxwant, b.nth + 1);
    }
    const size_t nq = source.npoints;
    if (nq == 0) return true;
    // the table in the order of the list widths (stable), and where each width's jobs start
    NNJobDev tab[NN_MAX_JOBS];
    int first_of[4] = {0, 0, 0, 0};
    int at = 0;
    for (int w = 0; w < 3; w++) {
        first_of[w] = at;
        for (int j = 0; j < njobs; j++) {
            const cwipc_hip_nn_job &b = jobs[j];
            if (nn_width_class(b.nth + 1) != w) continue;
            NNJobDev &d = tab[at++];
            d.max2 = b.max_distance * b.max_distance;
            d.src_y[0] = b.source_y[0]; d.src_y[1] = b.source_y[1];
            d.ref_y[0] = b.reference_y[0]; d.ref_y[1] = b.reference_y[1];
            d.row = (uint32_t)j;
            d.want = b.nth + 1;
            d.src_mask = b.source_mask;
            d.ref_mask = b.reference_mask;
        }
    }
    first_of[3] = at;
    // the caller's block: the table | two counts per job; the pinned staging holds the same
    const size_t tab_bytes = (size_t)njobs * sizeof(NNJobDev), cnt_bytes = (size_t)njobs * 2 * sizeof(uint32_t);
    char *block = (char *)dev_table;
    char *stage = (char *)c.staging(tab_bytes + cnt_bytes);
    if (!block || !stage) return false;
    const NNJobDev *dev_tab = (const NNJobDev *)block;
    uint32_t *dev_counts = (uint32_t *)(block + tab_bytes);
    memcpy(stage, tab, tab_bytes);
    if (hipMemcpyAsync(block, stage, tab_bytes, hipMemcpyHostToDevice, c.stream) != hipSuccess ||
        hipMemsetAsync(dev_counts, 0, cnt_bytes, c.stream) != hipSuccess) return false;
    CW_LAUNCH("nn_jobs_count", nn_jobs_count_kernel, dim3(std::min(grid_blocks(nq), 256u), (unsigned)njobs), dim3(GRID_BLK), 0, c.stream, source.y(),
              source.rgbt(), nq, dev_tab, 0, dev_counts);
    if (reference.npoints)
        CW_LAUNCH("nn_jobs_count", nn_jobs_count_kernel, dim3(std::min(grid_blocks(reference.npoints), 256u), (unsigned)njobs), dim3(GRID_BLK), 0, c.stream,
                  reference.y(), reference.rgbt(), reference.npoints, dev_tab, 1, dev_counts);
    if (hipGetLastError() != hipSuccess) return false;
    // the one wait of the search: which jobs have anybody on both sides
    if (hipMemcpyAsync(stage + tab_bytes, dev_counts, cnt_bytes, hipMemcpyDeviceToHost, c.stream) != hipSuccess || !c.sync()) return false;
    bool live[NN_MAX_JOBS];
    bool any_live = false;
    {
        const uint32_t *cnt = (const uint32_t *)(stage + tab_bytes);
        for (int e = 0; e < njobs; e++) {
            live[e] = cnt[2 * e] != 0 && cnt[2 * e + 1] != 0;
            any_live = any_live || live[e];
        }
    }
    NNJobsArgs A{};
    A.qx = source.x(); A.qy = source.y(); A.qz = source.z();
    A.qrgbt = source.rgbt();
    A.nq = nq;
    A.out = dev_out;
    // runs of consecutive table entries that are (not) searched: one launch each
    auto for_runs = [&](int lo, int hi, bool want_live, const std::function<void(int, int)> &f) {
        for (int e = lo; e < hi;) {
            if (live[e] != want_live) { e++; continue; }
            int end = e;
            while (end < hi && live[end] == want_live) end++;
            f(e, end - e);
            e = end;
        }
    };
    for_runs(0, njobs, false, [&](int e, int count) {
        NNJobsArgs F = A;
        F.jobs = dev_tab + e;
        CW_LAUNCH("nn_jobs_fill", nn_jobs_fill_kernel, dim3(std::min(grid_blocks(nq), 1024u), (unsigned)count), dim3(GRID_BLK), 0, c.stream, F);
    });
    if (hipGetLastError() != hipSuccess) return false;
    if (!any_live) return true;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        uint8_t *tiles = (uint8_t *)pool_alloc(v.n);
        if (!tiles) return false;
        tctx().free_later(tiles);
        CW_LAUNCH("nn_gather_tiles", nn_gather_tiles_kernel, dim3(grid_blocks(v.n)), dim3(GRID_BLK), 0, s, v.sorted, reference.rgbt(), v.n, reference.npoints, tiles);
        for (int w = 0; w < 3; w++)
            for_runs(first_of[w], first_of[w + 1], true, [&](int e, int count) {
                NNJobsArgs S = A;
                S.jobs = dev_tab + e;
                if (w == 0) launch_nn_jobs<2>(v, tiles, S, (unsigned)count, s);
                else if (w == 1) launch_nn_jobs<4>(v, tiles, S, (unsigned)count, s);
                else launch_nn_jobs<32>(v, tiles, S, (unsigned)count, s);
            });
        return hipGetLastError() == hipSuccess;
    };
    return grid_and_search(reference, std::max(maxwant, NN_GRID_WIDTH), true, search);
}

bool nn_distance2(const DeviceSoA &source, const DeviceSoA &reference, int nth, double max_distance, double *dev_out) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    const size_t nq = source.npoints;
    if (nq == 0) return true;
    if (nth < 0 || nth >= NN_MAX_NTH + 1 || !(max_distance > 0.0)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_nn_distance2", "nth must lie between 0 and 31, max_distance must be positive (inf: no bound)");
        return false;
    }
    if (reference.npoints == 0) {
        CW_LAUNCH("nn_fill_inf", nn_fill_inf_kernel, dim3(grid_blocks(nq)), dim3(GRID_BLK), 0, c.stream, dev_out, nq);
        return hipGetLastError() == hipSuccess;
    }
    NNArgs A{};
    A.qx = source.x(); A.qy = source.y(); A.qz = source.z();
    A.nq = nq;
    A.want = nth + 1;
    A.max2 = max_distance * max_distance;
    A.out = dev_out;
    const GridSearch search = [&](const GridView &v, hipStream_t s) {
        if (A.want <= 2) launch_nn<2>(v, A, s);
        else if (A.want <= 4) launch_nn<4>(v, A, s);
        else launch_nn<32>(v, A, s);
        return hipGetLastError() == hipSuccess;
    };
    // The grid's cell size: as for the outlier filter's k-NN of width 15 (about eight points to an occupied cell), of nth + 1 beyond.
    // The self-search's own choice for nth + 1 = 1 or 2 is a point or two per cell, right for queries that ARE reference points;
    // a query of another cloud may lie many cells from the nearest reference point (two camera tiles overlap along a seam
    // only), and until its first candidate turns up nothing bounds the shells it walks: (2r + 1)^2 rows of cells for shell r.
    // Cells 2.8 times as wide make that walk some twenty times shorter and give a near query a few dozen candidates more.
    return grid_and_search(reference, std::max(nth + 1, NN_GRID_WIDTH), true, search);
}

}  // namespace cwipc_amd
