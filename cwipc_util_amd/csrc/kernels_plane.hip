// kernels_plane.hip -- gfx950 kernels of plane segmentation (RULE S of include/cwipc_util_amd/hip_ext.h; the arithmetic is
// plane_seg_terms.hpp's, shared with the host twin).  No grid and no neighbour search: a dense points x hypotheses sweep with integer
// counts.
//
//   plane_hypotheses   one lane per hypothesis h: the triple, the plane through it, the validity word
//   plane_score        THE HOT KERNEL.  A workgroup (256 lanes) holds a tile of 2048 points in registers as f64, eight per lane, and
//                      walks the hypotheses: the four coefficients are wave-uniform (scalar loads from the table), per hypothesis
//                      eight predicates, eight ballots and popcounts, and one LDS add per wave.  The grid is persistent in both
//                      directions: workgroup (x, y) takes tiles x, x + grid.x, ... against the blocks of 64 hypotheses y,
//                      y + grid.y, ..., keeps a block's counts in LDS while it walks its tiles and writes them to row x of a
//                      [grid.x][H] table: no global atomics, nothing depends on scheduling.  grid.y is chosen so that a small
//                      cloud still fills the part (up to 2048 workgroups).
//   plane_colsum       counts[h] = the column sums of that table, sixteen lanes per column
//   plane_best         one workgroup: the valid hypothesis with the largest count, the smallest h on a tie; plane, anchor, triple and
//                      counts go to device memory, so that the refit follows without a host wait
//   plane_refit_sums   one pass over the points: ten 64-bit integer sums per lane over the best plane's inliers, reduced per wave and
//                      workgroup, then added to the best record with 64-bit integer vector atomics (integer adds commute: exact)
// The recount of a refit plane is plane_score with that one plane as an argument.  The partition by a plane is the floor partition's
// count / scan / scatter with a plane classifier (kernels_floor.hip).
#include "internal.hpp"
#include "plane_seg_terms.hpp"

namespace cwipc_amd {
namespace k {

static constexpr int PBLOCK = 256;
static constexpr int PWAVES = PBLOCK / 64;
static constexpr int PITEMS = PLANE_SCORE_TILE / PBLOCK;   // 8 points per lane: two dwordx4 per plane
static_assert(PITEMS == 8, "the score kernel loads two quads per lane and plane");
static_assert(PLANE_SCORE_HBLOCK <= PBLOCK, "a lane per LDS counter");

struct PlaneOne { double p[4]; };

__global__ void __launch_bounds__(PBLOCK) plane_hypotheses_kernel(PlaneRule r, const float *__restrict__ x, const float *__restrict__ y,
                                                                 const float *__restrict__ z, size_t n, double *__restrict__ planes,
                                                                 uint32_t *__restrict__ triples, uint32_t *__restrict__ valid) {
    const uint32_t h = blockIdx.x * PBLOCK + threadIdx.x;
    if (h >= r.iterations) return;
    uint32_t idx[3];
    plane_triple(r.base, h, (unsigned long long)n, idx);
    double plane[4] = {0.0, 0.0, 0.0, 0.0};
    bool ok = plane_triple_distinct(idx);   // (n == 0: three zeros, so nothing is loaded)
    if (ok) {
        double p[3][3];
        for (int k = 0; k < 3; k++) { p[k][0] = (double)x[idx[k]]; p[k][1] = (double)y[idx[k]]; p[k][2] = (double)z[idx[k]]; }
        ok = plane_through(r, p[0], p[1], p[2], plane);
    }
    for (int a = 0; a < 4; a++) planes[4 * (size_t)h + a] = plane[a];
    for (int k = 0; k < 3; k++) triples[3 * (size_t)h + k] = idx[k];
    valid[h] = ok ? 1u : 0u;
}

// four consecutive points of one plane from `base` on as doubles; beyond n a NaN, which is never an inlier
__device__ __forceinline__ void load_quad(const float *__restrict__ plane, size_t base, size_t n, double *v) {
    if (base + 4 <= n) {
        const float4 q = *reinterpret_cast<const float4 *>(plane + base);
        v[0] = (double)q.x; v[1] = (double)q.y; v[2] = (double)q.z; v[3] = (double)q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = base + j < n ? (double)plane[base + j] : (double)NAN;
    }
}

__global__ void __launch_bounds__(PBLOCK) plane_score_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                            const double *__restrict__ planes, const uint32_t *__restrict__ valid, uint32_t H,
                                                            PlaneOne one, int use_one, double distance, uint32_t *__restrict__ partial) {
    __shared__ uint32_t cnt[PLANE_SCORE_HBLOCK];
    const size_t ntiles = (n + PLANE_SCORE_TILE - 1) / PLANE_SCORE_TILE;
    const bool lane0 = (threadIdx.x & 63) == 0;
    // workgroup (x, y): the tiles x, x + gridDim.x, ... against the hypothesis blocks y, y + gridDim.y, ...
    for (uint32_t h0 = blockIdx.y * PLANE_SCORE_HBLOCK; h0 < H; h0 += gridDim.y * PLANE_SCORE_HBLOCK) {
        const uint32_t hn = H - h0 < (uint32_t)PLANE_SCORE_HBLOCK ? H - h0 : (uint32_t)PLANE_SCORE_HBLOCK;
        if (threadIdx.x < hn) cnt[threadIdx.x] = 0;
        __syncthreads();
        for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // (the trip count is the workgroup's)
            double px[PITEMS], py[PITEMS], pz[PITEMS];
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const size_t base = tile * PLANE_SCORE_TILE + (size_t)half * (PLANE_SCORE_TILE / 2) + (size_t)threadIdx.x * 4;
                load_quad(x, base, n, px + 4 * half);
                load_quad(y, base, n, py + 4 * half);
                load_quad(z, base, n, pz + 4 * half);
            }
            for (uint32_t j = 0; j < hn; j++) {
                double pl[4];
                if (use_one) {
#pragma unroll
                    for (int a = 0; a < 4; a++) pl[a] = one.p[a];
                } else {
                    const uint32_t h = h0 + j;
                    if (!valid[h]) continue;   // (uniform)
#pragma unroll
                    for (int a = 0; a < 4; a++) pl[a] = planes[4 * (size_t)h + a];
                }
                uint32_t c = 0;
#pragma unroll
                for (int i = 0; i < PITEMS; i++) c += (uint32_t)__popcll(__ballot(plane_inlier(plane_e(pl, px[i], py[i], pz[i]), distance)));
                if (c && lane0) atomicAdd(&cnt[j], c);   // (LDS, integer)
            }
        }
        __syncthreads();
        if (threadIdx.x < hn) partial[(size_t)blockIdx.x * H + h0 + threadIdx.x] = cnt[threadIdx.x];
        __syncthreads();
    }
}

// 64 columns per workgroup, sixteen lanes per column: lane (c, g) adds rows g, g + 16, ... of column c, LDS adds the sixteen
static constexpr int CGROUPS = 16;
__global__ void __launch_bounds__(64 * CGROUPS) plane_colsum_kernel(const uint32_t *__restrict__ partial, unsigned rows, uint32_t H, uint32_t *__restrict__ counts) {
    __shared__ uint32_t part[CGROUPS][64];
    const uint32_t col = threadIdx.x & 63, group = threadIdx.x >> 6, h = blockIdx.x * 64 + col;
    uint32_t c = 0;
    if (h < H)
        for (unsigned g = group; g < rows; g += CGROUPS) c += partial[(size_t)g * H + h];
    part[group][col] = c;
    __syncthreads();
    if (group == 0 && h < H) {
        for (int k = 1; k < CGROUPS; k++) c += part[k][col];
        counts[h] = c;
    }
}

__global__ void __launch_bounds__(PBLOCK) plane_best_kernel(const double *__restrict__ planes, const uint32_t *__restrict__ triples,
                                                           const uint32_t *__restrict__ valid, const uint32_t *__restrict__ counts, uint32_t H,
                                                           const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                           PlaneBest *__restrict__ best) {
    __shared__ unsigned long long wave_key[PWAVES];
    __shared__ uint32_t wave_valid[PWAVES];
    // count in the upper half, ~h in the lower: the largest key is the largest count and of those the smallest h; 0 is no key
    // (h < 65536, so a valid hypothesis never has ~h == 0)
    unsigned long long key = 0;
    uint32_t nvalid = 0;
    for (uint32_t h = threadIdx.x; h < H; h += PBLOCK) {
        if (!valid[h]) continue;
        nvalid++;
        const unsigned long long kk = ((unsigned long long)counts[h] << 32) | (unsigned long long)(0xffffffffu - h);
        key = kk > key ? kk : key;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o > key ? o : key;
        nvalid += __shfl_down(nvalid, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { wave_key[threadIdx.x >> 6] = key; wave_valid[threadIdx.x >> 6] = nvalid; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < PWAVES; w++) {
        key = wave_key[w] > key ? wave_key[w] : key;
        nvalid += wave_valid[w];
    }
    PlaneBest b;
    for (int a = 0; a < 4; a++) b.plane[a] = 0.0;
    for (int a = 0; a < 3; a++) { b.anchor[a] = 0.0; b.triple[a] = 0; }
    b.h = b.count = 0;
    b.pad = 0;
    b.nvalid = nvalid;
    b.found = key != 0ull ? 1u : 0u;
    if (b.found) {
        b.h = 0xffffffffu - (uint32_t)key;
        b.count = (uint32_t)(key >> 32);
        for (int a = 0; a < 4; a++) b.plane[a] = planes[4 * (size_t)b.h + a];
        for (int a = 0; a < 3; a++) b.triple[a] = triples[3 * (size_t)b.h + a];
        b.anchor[0] = (double)x[b.triple[0]]; b.anchor[1] = (double)y[b.triple[0]]; b.anchor[2] = (double)z[b.triple[0]];
    }
    for (int i = 0; i < 10; i++) b.sums[i] = 0ull;
    *best = b;
}

__global__ void __launch_bounds__(PBLOCK) plane_refit_sums_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                                 double distance, PlaneBest *__restrict__ best) {
    __shared__ unsigned long long red[PWAVES][10];
    if (!best->found) return;   // (uniform)
    double plane[4], anchor[3];
    for (int a = 0; a < 4; a++) plane[a] = best->plane[a];
    for (int a = 0; a < 3; a++) anchor[a] = best->anchor[a];
    const double s = rn_div(PLANE_FIX, distance);
    uint64_t v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * PBLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * PBLOCK) {
        const double p[3] = {(double)x[i], (double)y[i], (double)z[i]};
        if (!plane_inlier(plane_e(plane, p[0], p[1], p[2]), distance)) continue;
        int64_t o[3];
        if (plane_offsets(p, anchor, s, o)) plane_sums_add(v, o);
    }
#pragma unroll
    for (int t = 0; t < 10; t++) {
        unsigned long long w = v[t];
        for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][t] = w;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        unsigned long long w = 0;
        for (int k = 0; k < PWAVES; k++) w += red[k][threadIdx.x];
        if (w) atomicAdd(&best->sums[threadIdx.x], w);
    }
}

unsigned plane_score_grid(size_t n, uint32_t H) {
    size_t g = (n + PLANE_SCORE_TILE - 1) / PLANE_SCORE_TILE;
    const size_t room = ((size_t)4 << 20) / (H ? H : 1);   // the partial table stays within 4 M words
    if (g > room) g = room;
    if (g > (size_t)PLANE_SCORE_GRID) g = PLANE_SCORE_GRID;
    if (g < 1) g = 1;
    return (unsigned)g;
}

static inline size_t up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

size_t plane_work_bytes(size_t n, uint32_t H) {
    return up256((size_t)H * 32) + 3 * up256((size_t)H * 4) + up256((size_t)H * 12) + up256(sizeof(PlaneBest)) + up256((size_t)plane_score_grid(n, H) * H * 4);
}

void plane_work_layout(void *block, size_t n, uint32_t H, PlaneWork &w) {
    char *at = (char *)block;
    w.planes = (double *)at;      at += up256((size_t)H * 32);
    w.triples = (uint32_t *)at;   at += up256((size_t)H * 12);
    w.valid = (uint32_t *)at;     at += up256((size_t)H * 4);
    w.counts = (uint32_t *)at;    at += up256((size_t)H * 4);
    w.best = (PlaneBest *)at;     at += up256(sizeof(PlaneBest));
    w.partial = (uint32_t *)at;
    w.grid = plane_score_grid(n, H);
}

void plane_hypotheses(const DeviceSoA &src, const PlaneRule &r, const PlaneWork &w, hipStream_t s) {
    const float *x = src.npoints ? src.x() : nullptr, *y = src.npoints ? src.y() : nullptr, *z = src.npoints ? src.z() : nullptr;
    CW_LAUNCH("plane_hypotheses", plane_hypotheses_kernel, dim3((r.iterations + PBLOCK - 1) / PBLOCK), dim3(PBLOCK), 0, s, r, x, y, z, src.npoints, w.planes,
              w.triples, w.valid);
}

void plane_score(const DeviceSoA &src, double distance, uint32_t H, const PlaneWork &w, const double *one, hipStream_t s) {
    const float *x = src.npoints ? src.x() : nullptr, *y = src.npoints ? src.y() : nullptr, *z = src.npoints ? src.z() : nullptr;
    PlaneOne arg = {{0.0, 0.0, 0.0, 0.0}};
    if (one) for (int a = 0; a < 4; a++) arg.p[a] = one[a];
    const uint32_t cols = one ? 1u : H;
    // (the grid is the layout's: the recount uses the same rows, one column of them)
    // enough workgroups for eight per CU where points and hypotheses allow it: the hypothesis blocks spread over grid.y
    const unsigned blocks = (cols + PLANE_SCORE_HBLOCK - 1) / PLANE_SCORE_HBLOCK, want = w.grid >= 2048 ? 1u : 2048u / w.grid;
    CW_LAUNCH("plane_score", plane_score_kernel, dim3(w.grid, blocks < want ? blocks : want), dim3(PBLOCK), 0, s, x, y, z, src.npoints, (const double *)w.planes, (const uint32_t *)w.valid, cols,
              arg, one ? 1 : 0, distance, w.partial);
    CW_LAUNCH("plane_colsum", plane_colsum_kernel, dim3((cols + 63) / 64), dim3(64 * CGROUPS), 0, s, (const uint32_t *)w.partial, w.grid, cols, w.counts);
}

void plane_best(const DeviceSoA &src, uint32_t H, const PlaneWork &w, hipStream_t s) {
    const float *x = src.npoints ? src.x() : nullptr, *y = src.npoints ? src.y() : nullptr, *z = src.npoints ? src.z() : nullptr;
    CW_LAUNCH("plane_best", plane_best_kernel, dim3(1), dim3(PBLOCK), 0, s, (const double *)w.planes, (const uint32_t *)w.triples, (const uint32_t *)w.valid,
              (const uint32_t *)w.counts, H, x, y, z, w.best);
}

void plane_refit_sums(const DeviceSoA &src, double distance, const PlaneWork &w, hipStream_t s) {
    if (!src.npoints) return;
    size_t g = (src.npoints + 4 * PBLOCK - 1) / (4 * PBLOCK);
    if (g > 512) g = 512;
    CW_LAUNCH("plane_refit_sums", plane_refit_sums_kernel, dim3((unsigned)g), dim3(PBLOCK), 0, s, src.x(), src.y(), src.z(), src.npoints, distance, w.best);
}

}  // namespace k
}  // namespace cwipc_amd
