// kernels_markers.hip -- gfx950 kernels of cwipc_hip_detect_markers: an rgb image in, the ids and corners of the square binary
// fiducials in it out (5 x 5 payload inside a one-cell black border, a 7 x 7 grid: the family of the reference's printable targets,
// data/src/5x5_1000-N.svg, which the reference finds with cv2.aruco in python/cwipc/registration/multicoarse.py:492-527).
//
// The contract (include/cwipc_util_amd/hip_ext.h has it in full; tests/marker_model.py is its numpy model).  Every step is integer
// arithmetic, so the model and these kernels agree bit for bit.  w = window_half, r = row, c = column, linear index = r*width + c:
//   1. grey        Y = (77*R + 150*G + 29*B + 128) >> 8
//   2. dark mask   S = sum of Y over [r-w, r+w] x [c-w, c+w] clipped to the image, n = that window's pixel count;
//                  dark iff Y*n + threshold_offset*n < S.  S comes from a summed-area table in uint32 (255 * 2^24 fits).
//   3. components  4-connected sets of dark pixels; a component's label is its smallest linear index
//   4. candidate   the bounding box touches no image edge and is at least min_side wide and high
//   5. corners     P0 = the label's pixel; A = the component pixel farthest from P0 (squared distance); C = the one farthest from
//                  A; k(p) = (px-Ax)*(Cy-Ay) - (py-Ay)*(Cx-Ax); B = largest k, D = smallest k; every tie to the smallest linear
//                  index.  Rejected unless k(B) > 0 > k(D) and A, B, C, D is strictly convex.  Q0..Q3 = the cycle from A in the
//                  direction whose shoelace sum is positive (clockwise on screen, y runs down).
//                  Limit: this finds the corners of a quadrilateral whose diagonals are longer than its sides, no other.
//   6. sampling    the projective map of the square (0,0), (7,0), (7,7), (0,7) onto Q0..Q3 (Heckbert's closed form, see
//                  marker_map); cell (i, j) is sampled at (j + a/4, i + b/4), a, b in {1, 2, 3}; a sample's pixel is
//                  floor(num/den + 1/2) per coordinate by exact integer division; black iff >= 5 of the 9 pixels are dark, a
//                  sample outside the image is not dark.
//   7. decode      rejected if more than max_border_errors of the 24 border cells are white; the 25 inner cells, white = 1, are
//                  compared in the four rotations with dictionary[id] & 0x1FFFFFF (bit 24 - (5*row + col)); rotation k: the
//                  marker's top-left corner is Q_k; smallest Hamming distance, ties to the smallest id, then the smallest k;
//                  accepted iff the distance is <= max_bit_errors; corners out: Q_k, Q_(k+1), Q_(k+2), Q_(k+3).
//   8. output      per id the candidate of largest area (ties: smallest label), sorted by id (host side, render.cpp).
//
// Magnitudes, L = the larger image side.  Coordinates are < L, so squared distances and |k| are < 2 L^2 and are packed into 32 bits
// (k with a bias of 2^31): L <= 2^14 keeps them below 2^29.  In the map, |Dn| < 2 L^2, |G|, |H| < 4 L^2, the numerator
// coefficients are < 6 L^3, 6 L^3 and 2 L^3, a numerator with U, V <= 27 is < (27*6 + 27*6 + 28*2) L^3 = 380 L^3 and the
// denominator < (27*4 + 27*4 + 28*2) L^2 = 272 L^2; the rounding divides 2*num + den, < 760 L^3 + 272 L^2, by 2*den.  int64 holds
// that for L <= 2^17.  The entry points refuse a side above MARKER_MAX_SIDE = 8192: 760 * 2^39 + 272 * 2^26 < 2^49.
//
// Kernels: grey + row scan, column scan, threshold (+ union-find initialisation), merge, flatten, per-label area and bounding
// box, candidate list, three extreme-point passes, decode (one wave per candidate).  Launches on one stream are ordered, and one
// kernel's stores are visible to the next; inside the merge and the flatten kernel, the only ones in which workgroups read what
// others write (the finds halve paths), every access to a dark pixel's word of the parent array is an agent-scope atomic.
#include "internal.hpp"
#include "block_scan.hpp"
#include "union_find.hpp"

namespace cwipc_amd {
namespace k {

static constexpr int MBLOCK = 256;
static constexpr uint32_t MNONE = 0xFFFFFFFFu;

static inline unsigned marker_grid(size_t items) {
    size_t g = (items + MBLOCK - 1) / MBLOCK;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;
    return (unsigned)g;
}

// ---- 1. grey and the summed-area table ----
// One workgroup per row: grey[r][c] and the row's inclusive prefix sums into sat.  The loop's trip count depends on width alone, so
// every lane reaches every barrier.
__global__ void __launch_bounds__(MBLOCK) marker_grey_rows_kernel(const uint8_t *__restrict__ rgb, int width, int height, uint8_t *__restrict__ grey,
                                                                 uint32_t *__restrict__ sat) {
    __shared__ uint32_t wave_sum[MBLOCK / 64];
    for (int r = blockIdx.x; r < height; r += gridDim.x) {
        uint32_t carry = 0;
        for (int base = 0; base < width; base += MBLOCK) {
            const int c = base + (int)threadIdx.x;
            uint32_t y = 0;
            if (c < width) {
                const uint8_t *p = rgb + ((size_t)r * width + c) * 3;
                y = (77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8;
                grey[(size_t)r * width + c] = (uint8_t)y;
            }
            uint32_t total;
            const uint32_t before = block_exclusive_scan<MBLOCK>(y, wave_sum, &total);
            if (c < width) sat[(size_t)r * width + c] = carry + before + y;
            carry += total;
            __syncthreads();   // wave_sum is written again in the next step
        }
    }
}

// One lane per column, eight rows in flight: the loads of a step are issued before its dependent adds.
__global__ void __launch_bounds__(MBLOCK) marker_sat_columns_kernel(int width, int height, uint32_t *__restrict__ sat) {
    const int c = blockIdx.x * MBLOCK + threadIdx.x;
    if (c >= width) return;
    uint32_t acc = 0;
    int r = 0;
    for (; r + 8 <= height; r += 8) {
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = sat[(size_t)(r + j) * width + c];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            acc += v[j];
            sat[(size_t)(r + j) * width + c] = acc;
        }
    }
    for (; r < height; r++) {
        acc += sat[(size_t)r * width + c];
        sat[(size_t)r * width + c] = acc;
    }
}

// ---- 2. threshold; parent[i] = i for a dark pixel, MNONE for a light one; *ncand = 0 ----
__global__ void __launch_bounds__(MBLOCK) marker_threshold_kernel(const uint8_t *__restrict__ grey, const uint32_t *__restrict__ sat, int width, int height,
                                                                 int w, int offset, uint8_t *__restrict__ dark, uint32_t *__restrict__ parent,
                                                                 uint32_t *__restrict__ ncand) {
    const size_t npix = (size_t)width * height, stride = (size_t)gridDim.x * MBLOCK;
    if (blockIdx.x == 0 && threadIdx.x == 0) *ncand = 0;
    for (size_t i = (size_t)blockIdx.x * MBLOCK + threadIdx.x; i < npix; i += stride) {
        const int r = (int)(i / width), c = (int)(i % width);
        const int r0 = r - w < 0 ? 0 : r - w, r1 = r + w > height - 1 ? height - 1 : r + w;
        const int c0 = c - w < 0 ? 0 : c - w, c1 = c + w > width - 1 ? width - 1 : c + w;
        // the four table corners; those above the first row or left of the first column are 0.  uint32 wraps, the result fits.
        uint32_t s = sat[(size_t)r1 * width + c1];
        if (r0 > 0) s -= sat[(size_t)(r0 - 1) * width + c1];
        if (c0 > 0) s -= sat[(size_t)r1 * width + (c0 - 1)];
        if (r0 > 0 && c0 > 0) s += sat[(size_t)(r0 - 1) * width + (c0 - 1)];
        const int64_t n = (int64_t)(r1 - r0 + 1) * (c1 - c0 + 1);
        const bool d = (int64_t)grey[i] * n + (int64_t)offset * n < (int64_t)s;
        dark[i] = d ? 1 : 0;
        parent[i] = d ? (uint32_t)i : MNONE;
    }
}

// ---- 3. union-find ----
// The atomic union-find of union_find.hpp (its invariant, termination and correctness arguments are written there): parent[x] <= x
// for every dark x at all times -- it holds after the threshold kernel (parent[x] = x) -- and a light pixel's MNONE is never reached
// from a dark one.
__device__ inline uint32_t marker_find(uint32_t *parent, uint32_t x) {
    UfDeviceAtomics at;
    return uf_find(parent, x, at);
}
__device__ inline void marker_union(uint32_t *parent, uint32_t a, uint32_t b) {
    UfDeviceAtomics at;
    (void)uf_union(parent, a, b, at);
}

__global__ void __launch_bounds__(MBLOCK) marker_merge_kernel(const uint8_t *__restrict__ dark, int width, int height, uint32_t *parent) {
    const size_t npix = (size_t)width * height, stride = (size_t)gridDim.x * MBLOCK;
    for (size_t i = (size_t)blockIdx.x * MBLOCK + threadIdx.x; i < npix; i += stride) {
        if (!dark[i]) continue;
        const int r = (int)(i / width), c = (int)(i % width);
        if (c + 1 < width && dark[i + 1]) marker_union(parent, (uint32_t)i, (uint32_t)(i + 1));
        if (r + 1 < height && dark[i + width]) marker_union(parent, (uint32_t)i, (uint32_t)(i + width));
    }
}

// label[i] = the root of i's tree, the component's smallest index (every member's chain of parents ends at the root and never
// rises, so the root is <= every member and is a member itself).  The merge kernel is done: the finds here only halve paths.
// A root's area and bounding box are set to their neutral values.
__global__ void __launch_bounds__(MBLOCK) marker_flatten_kernel(uint32_t *parent, size_t npix, uint32_t *__restrict__ label, uint32_t *__restrict__ area,
                                                               uint32_t *__restrict__ box /* 4 planes: min c, min r, max c, max r */) {
    const size_t stride = (size_t)gridDim.x * MBLOCK;
    for (size_t i = (size_t)blockIdx.x * MBLOCK + threadIdx.x; i < npix; i += stride) {
        uint32_t l = MNONE;
        if (parent[i] != MNONE) l = marker_find(parent, (uint32_t)i);
        label[i] = l;
        if (l == (uint32_t)i) {
            area[i] = 0;
            box[i] = MNONE; box[npix + i] = MNONE; box[2 * npix + i] = 0; box[3 * npix + i] = 0;
        }
    }
}

// ---- wave helpers.  Every caller's loop runs the same number of steps in all 64 lanes (marker_steps), so all lanes are there. ----
__device__ inline size_t marker_steps(size_t npix, size_t stride) { return (npix + stride - 1) / stride; }

// true when at least one lane has a label and all that have one have the same: *lead = that label
__device__ inline bool marker_wave_shares(uint32_t label, uint32_t *lead) {
    const unsigned long long m = __ballot(label != MNONE);
    if (m == 0) { *lead = MNONE; return false; }
    *lead = __shfl(label, __ffsll((long long)m) - 1, 64);
    return __all(label == MNONE || label == *lead);
}
__device__ inline uint32_t wave_min_u32(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
__device__ inline uint32_t wave_max_u32(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}
__device__ inline unsigned long long wave_max_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}
__device__ inline unsigned long long wave_min_u64(unsigned long long v) { return ~wave_max_u64(~v); }

// ---- 4. per-label area and bounding box.  Consecutive lanes are consecutive pixels of a row: where a wave's dark lanes share
// their label, the common case, the wave reduces first and one lane issues the five atomics. ----
__global__ void __launch_bounds__(MBLOCK) marker_stats_kernel(const uint32_t *__restrict__ label, int width, size_t npix, uint32_t *area, uint32_t *box) {
    const size_t stride = (size_t)gridDim.x * MBLOCK, steps = marker_steps(npix, stride);
    size_t i = (size_t)blockIdx.x * MBLOCK + threadIdx.x;
    for (size_t step = 0; step < steps; step++, i += stride) {
        const uint32_t l = i < npix ? label[i] : MNONE;
        const uint32_t c = i < npix ? (uint32_t)(i % width) : 0, r = i < npix ? (uint32_t)(i / width) : 0;
        uint32_t lead;
        if (marker_wave_shares(l, &lead)) {
            const bool in = l != MNONE;
            const uint32_t cnt = (uint32_t)__popcll(__ballot(in));
            const uint32_t c0 = wave_min_u32(in ? c : MNONE), r0 = wave_min_u32(in ? r : MNONE);
            const uint32_t c1 = wave_max_u32(in ? c : 0), r1 = wave_max_u32(in ? r : 0);
            if ((threadIdx.x & 63) == 0) {
                atomicAdd(area + lead, cnt);
                atomicMin(box + lead, c0); atomicMin(box + npix + lead, r0);
                atomicMax(box + 2 * npix + lead, c1); atomicMax(box + 3 * npix + lead, r1);
            }
        } else if (l != MNONE) {
            atomicAdd(area + l, 1u);
            atomicMin(box + l, c); atomicMin(box + npix + l, r);
            atomicMax(box + 2 * npix + l, c); atomicMax(box + 3 * npix + l, r);
        }
    }
}

// ---- 5. candidates: slot[root] = its place in the list (the order of the list is arbitrary, nothing that goes out depends on it),
// MNONE for a component that is none.  A candidate has at least 2*min_side - 1 pixels, which bounds the list (cap). ----
__global__ void __launch_bounds__(MBLOCK) marker_candidates_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ box, int width, int height,
                                                                  int min_side, uint32_t cap, uint32_t *__restrict__ slot, uint32_t *ncand,
                                                                  uint32_t *__restrict__ cand_label, unsigned long long *__restrict__ keys /* 4 planes of cap */) {
    const size_t npix = (size_t)width * height, stride = (size_t)gridDim.x * MBLOCK;
    for (size_t i = (size_t)blockIdx.x * MBLOCK + threadIdx.x; i < npix; i += stride) {
        if (label[i] != (uint32_t)i) continue;
        const uint32_t c0 = box[i], r0 = box[npix + i], c1 = box[2 * npix + i], r1 = box[3 * npix + i];
        uint32_t s = MNONE;
        if (c0 > 0 && r0 > 0 && c1 < (uint32_t)width - 1 && r1 < (uint32_t)height - 1 && c1 - c0 + 1 >= (uint32_t)min_side && r1 - r0 + 1 >= (uint32_t)min_side) {
            s = atomicAdd(ncand, 1u);
            if (s < cap) {   // (always, by the bound on the list; checked because a store depends on it)
                cand_label[s] = (uint32_t)i;
                keys[s] = 0; keys[cap + s] = 0; keys[2 * (size_t)cap + s] = 0; keys[3 * (size_t)cap + s] = 0;
            } else {
                s = MNONE;
            }
        }
        slot[i] = s;
    }
}

// ---- 6. the extreme points: per candidate the maximum of value << 32 | ~index (largest value, among equals the smallest index).
// pass 0: A, value = squared distance from P0 (the label's pixel); pass 1: C, from A (read from plane 0);
// pass 2: B, value = k + 2^31 into plane 2, and D, value = 2^31 - k into plane 3, k as at the top (A and C from planes 0 and 1). ----
__device__ inline void marker_point_of_key(unsigned long long key, int width, int *x, int *y) {
    const uint32_t idx = ~(uint32_t)key;
    *x = (int)(idx % (uint32_t)width);
    *y = (int)(idx / (uint32_t)width);
}

template <int PASS>
__global__ void __launch_bounds__(MBLOCK) marker_extreme_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ slot, int width, size_t npix,
                                                               uint32_t cap, unsigned long long *keys) {
    const size_t stride = (size_t)gridDim.x * MBLOCK, steps = marker_steps(npix, stride);
    size_t i = (size_t)blockIdx.x * MBLOCK + threadIdx.x;
    for (size_t step = 0; step < steps; step++, i += stride) {
        uint32_t l = i < npix ? label[i] : MNONE;
        uint32_t s = MNONE;
        if (l != MNONE) s = slot[l];
        if (s == MNONE) l = MNONE;   // not a candidate's pixel
        unsigned long long k0 = 0, k1 = 0;
        if (l != MNONE) {
            const int px = (int)(i % width), py = (int)(i / width);
            const unsigned long long low = (unsigned long long)(~(uint32_t)i);
            if (PASS == 0) {
                const int dx = px - (int)(l % (uint32_t)width), dy = py - (int)(l / (uint32_t)width);
                k0 = ((unsigned long long)(uint32_t)(dx * dx + dy * dy) << 32) | low;
            } else if (PASS == 1) {
                int ax, ay;
                marker_point_of_key(keys[s], width, &ax, &ay);   // plane 0 is final: written by the launch before this one
                const int dx = px - ax, dy = py - ay;
                k0 = ((unsigned long long)(uint32_t)(dx * dx + dy * dy) << 32) | low;
            } else {
                int ax, ay, cx, cy;
                marker_point_of_key(keys[s], width, &ax, &ay);
                marker_point_of_key(keys[cap + s], width, &cx, &cy);
                const int kk = (px - ax) * (cy - ay) - (py - ay) * (cx - ax);
                k0 = ((unsigned long long)(0x80000000u + (uint32_t)kk) << 32) | low;
                k1 = ((unsigned long long)(0x80000000u - (uint32_t)kk) << 32) | low;
            }
        }
        const size_t plane = PASS == 0 ? 0 : PASS == 1 ? (size_t)cap : 2 * (size_t)cap;
        uint32_t lead;
        if (marker_wave_shares(l, &lead)) {
            // every lane with a label has the label `lead`, hence one slot; lanes without one hold the neutral key 0
            const uint32_t ls = slot[lead];
            k0 = wave_max_u64(k0);
            if (PASS == 2) k1 = wave_max_u64(k1);
            if ((threadIdx.x & 63) == 0) {
                atomicMax(keys + plane + ls, k0);
                if (PASS == 2) atomicMax(keys + 3 * (size_t)cap + ls, k1);
            }
        } else if (l != MNONE) {
            atomicMax(keys + plane + s, k0);
            if (PASS == 2) atomicMax(keys + 3 * (size_t)cap + s, k1);
        }
    }
}

// ---- 7. decode ----
// The projective map of the unit square onto the quadrilateral (x0,y0)..(x3,y3) (Heckbert, "Fundamentals of texture mapping and
// image warping", 1989, section 2.2.3), all over the common denominator Dn:
//   dx1 = x1-x2, dx2 = x3-x2, sx = x0-x1+x2-x3 (dy1, dy2, sy alike);  Dn = dx1*dy2 - dx2*dy1, G = sx*dy2 - dx2*sy, H = dx1*sy - sx*dy1
//   x(u, v) = ((x1-x0)*Dn + G*x1) u + ((x3-x0)*Dn + H*x3) v + x0*Dn  over  G u + H v + Dn  (y alike).
// With u = U/28, v = V/28 (U = 4j + a, V = 4i + b: the square of side 7 in quarter cells) everything is multiplied by 28.
struct MarkerMap {
    int64_t ax, bx, cx, ay, by, cy, g, h, dn;
};
__device__ inline MarkerMap marker_map(const int qx[4], const int qy[4]) {
    const int64_t x0 = qx[0], x1 = qx[1], x2 = qx[2], x3 = qx[3], y0 = qy[0], y1 = qy[1], y2 = qy[2], y3 = qy[3];
    const int64_t dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3, dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
    MarkerMap m;
    m.dn = dx1 * dy2 - dx2 * dy1;
    m.g = sx * dy2 - dx2 * sy;
    m.h = dx1 * sy - sx * dy1;
    m.ax = (x1 - x0) * m.dn + m.g * x1; m.bx = (x3 - x0) * m.dn + m.h * x3; m.cx = x0 * m.dn;
    m.ay = (y1 - y0) * m.dn + m.g * y1; m.by = (y3 - y0) * m.dn + m.h * y3; m.cy = y0 * m.dn;
    return m;
}
__device__ inline int64_t marker_floor_div(int64_t a, int64_t b /* > 0 */) {
    int64_t q = a / b;
    if (a % b < 0) q--;
    return q;
}

// the 5 x 5 code read with Q_k as the top-left corner, from the code read with Q_0 there (bit 24 - (5*row + col)):
// k = 1: canonical (r, c) is observed (c, 4-r); k = 2: (4-r, 4-c); k = 3: (4-c, r)
__device__ inline uint32_t marker_rotate_code(uint32_t code, int k) {
    uint32_t out = 0;
    for (int r = 0; r < 5; r++)
        for (int c = 0; c < 5; c++) {
            const int i = k == 0 ? r : k == 1 ? c : k == 2 ? 4 - r : 4 - c;
            const int j = k == 0 ? c : k == 1 ? 4 - r : k == 2 ? 4 - c : r;
            out |= ((code >> (24 - (5 * i + j))) & 1u) << (24 - (5 * r + c));
        }
    return out;
}

// One wave per candidate.  All lanes compute the quadrilateral (a few dozen integer operations on wave-uniform values), lane
// 7*i + j < 49 samples cell (i, j), the ballot gathers the cells, the lanes share the dictionary among them and a wave minimum
// of distance << 32 | id << 2 | k picks the match.
__global__ void __launch_bounds__(64) marker_decode_kernel(const uint8_t *__restrict__ dark, int width, int height, const uint32_t *__restrict__ ncand, uint32_t cap,
                                                          const uint32_t *__restrict__ cand_label, const unsigned long long *__restrict__ keys,
                                                          const uint32_t *__restrict__ area, const uint32_t *__restrict__ dictionary, int nmarkers,
                                                          int max_border_errors, int max_bit_errors, const float *__restrict__ depth /* or nullptr */,
                                                          MarkerRecord *__restrict__ records) {
    const int lane = threadIdx.x;
    uint32_t n = *ncand;
    if (n > cap) n = cap;
    for (uint32_t s = blockIdx.x; s < n; s += gridDim.x) {   // s and n are the same in every lane
        const uint32_t root = cand_label[s];
        MarkerRecord rec;
        rec.id = -1; rec.area = area[root]; rec.label = root; rec.pad = 0;
        for (int q = 0; q < 4; q++) { rec.x[q] = 0; rec.y[q] = 0; rec.depth[q] = 0.0f; }
        const unsigned long long kb = keys[2 * (size_t)cap + s], kd = keys[3 * (size_t)cap + s];
        const int32_t k_of_b = (int32_t)((uint32_t)(kb >> 32) - 0x80000000u), k_of_d = (int32_t)(0x80000000u - (uint32_t)(kd >> 32));
        int px[4], py[4];
        marker_point_of_key(keys[s], width, &px[0], &py[0]);
        marker_point_of_key(kb, width, &px[1], &py[1]);
        marker_point_of_key(keys[cap + s], width, &px[2], &py[2]);
        marker_point_of_key(kd, width, &px[3], &py[3]);
        bool ok = k_of_b > 0 && k_of_d < 0;
        int pos = 0, neg = 0;
        int64_t shoelace = 0;
        for (int q = 0; q < 4; q++) {
            const int q1 = (q + 1) & 3, q2 = (q + 2) & 3;
            const int64_t cr = (int64_t)(px[q1] - px[q]) * (py[q2] - py[q1]) - (int64_t)(py[q1] - py[q]) * (px[q2] - px[q1]);
            pos += cr > 0; neg += cr < 0;
            shoelace += (int64_t)px[q] * py[q1] - (int64_t)px[q1] * py[q];
        }
        ok = ok && (pos == 4 || neg == 4);
        int qx[4], qy[4];
        for (int q = 0; q < 4; q++) {
            const int from = shoelace > 0 ? q : (4 - q) & 3;
            qx[q] = px[from]; qy[q] = py[from];
        }
        const MarkerMap m = marker_map(qx, qy);
        if (ok) {   // (uniform)
            bool black = false;
            if (lane < 49) {
                const int i = lane / 7, j = lane % 7;
                int count = 0;
                for (int b = 1; b <= 3; b++)
                    for (int a = 1; a <= 3; a++) {
                        const int64_t U = 4 * j + a, V = 4 * i + b;
                        int64_t den = m.g * U + m.h * V + m.dn * 28;
                        int64_t nx = m.ax * U + m.bx * V + m.cx * 28, ny = m.ay * U + m.by * V + m.cy * 28;
                        if (den < 0) { den = -den; nx = -nx; ny = -ny; }
                        if (den == 0) continue;   // (not for a strictly convex quadrilateral; such a sample is not dark)
                        const int64_t sxp = marker_floor_div(2 * nx + den, 2 * den), syp = marker_floor_div(2 * ny + den, 2 * den);
                        if (sxp >= 0 && sxp < width && syp >= 0 && syp < height) count += dark[(size_t)syp * width + (size_t)sxp];
                    }
                black = count >= 5;
            }
            const unsigned long long cells = __ballot(black);   // bit 7*i + j
            int border_white = 0;
            uint32_t code = 0;
            for (int i = 0; i < 7; i++)
                for (int j = 0; j < 7; j++) {
                    const uint32_t white = (uint32_t)((~cells >> (7 * i + j)) & 1ull);
                    if (i == 0 || i == 6 || j == 0 || j == 6) border_white += (int)white;
                    else code |= white << (24 - (5 * (i - 1) + (j - 1)));
                }
            if (border_white <= max_border_errors) {
                uint32_t rot[4];
                for (int k = 0; k < 4; k++) rot[k] = marker_rotate_code(code, k);
                unsigned long long best = ~0ull;
                for (int id = lane; id < nmarkers; id += 64) {
                    const uint32_t word = dictionary[id] & 0x1FFFFFFu;
                    for (int k = 0; k < 4; k++) {
                        const unsigned long long cand = ((unsigned long long)__popc(rot[k] ^ word) << 32) | ((unsigned long long)(uint32_t)id << 2) | (uint32_t)k;
                        best = cand < best ? cand : best;
                    }
                }
                best = wave_min_u64(best);
                if ((int)(best >> 32) <= max_bit_errors) {
                    const int k = (int)(best & 3);
                    rec.id = (int32_t)((uint32_t)best >> 2);
                    for (int q = 0; q < 4; q++) {
                        rec.x[q] = qx[(q + k) & 3]; rec.y[q] = qy[(q + k) & 3];
                        if (depth) rec.depth[q] = depth[(size_t)rec.y[q] * width + rec.x[q]];   // a component's pixel: inside the image
                    }
                }
            }
        }
        if (lane == 0) records[s] = rec;
    }
}

// labels for the parity tests: the label as int32, -1 for a light pixel
__global__ void __launch_bounds__(MBLOCK) marker_labels_out_kernel(const uint32_t *__restrict__ label, size_t npix, int32_t *__restrict__ out) {
    const size_t stride = (size_t)gridDim.x * MBLOCK;
    for (size_t i = (size_t)blockIdx.x * MBLOCK + threadIdx.x; i < npix; i += stride) out[i] = label[i] == MNONE ? -1 : (int32_t)label[i];
}

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

uint32_t marker_candidate_cap(size_t npix, int min_side) { return (uint32_t)(npix / (size_t)(2 * min_side - 1) + 1); }

size_t marker_workspace_bytes(size_t npix, int min_side, int nmarkers) {
    const size_t cap = marker_candidate_cap(npix, min_side);
    // grey | dark | sat (later: slot) | parent | label | area | box x 4 | ncand | cand_label | keys x 4 | records | dictionary
    return 2 * up256(npix) + 4 * up256(npix * 4) + up256(npix * 16) + 256 + up256(cap * 4) + up256(cap * 32) + up256(cap * sizeof(MarkerRecord)) + up256((size_t)nmarkers * 4);
}

MarkerWorkspace marker_launch(const uint8_t *dev_rgb, int width, int height, const uint32_t *dict_staged, int nmarkers, const cwipc_hip_marker_params &p,
                              const float *dev_depth, void *workspace, hipStream_t s) {
    const size_t npix = (size_t)width * height;
    const uint32_t cap = marker_candidate_cap(npix, p.min_side);
    uint8_t *at = (uint8_t *)workspace;
    auto take = [&at](size_t bytes) { uint8_t *rv = at; at += up256(bytes); return rv; };
    uint8_t *grey = take(npix), *dark = take(npix);
    uint32_t *sat = (uint32_t *)take(npix * 4), *parent = (uint32_t *)take(npix * 4), *label = (uint32_t *)take(npix * 4);
    uint32_t *area = (uint32_t *)take(npix * 4), *box = (uint32_t *)take(npix * 16);
    uint32_t *ncand = (uint32_t *)take(256), *cand_label = (uint32_t *)take((size_t)cap * 4);
    unsigned long long *keys = (unsigned long long *)take((size_t)cap * 32);
    MarkerRecord *records = (MarkerRecord *)take((size_t)cap * sizeof(MarkerRecord));
    uint32_t *dict = (uint32_t *)take((size_t)nmarkers * 4);
    uint32_t *slot = sat;   // the table is not read after the threshold kernel
    MarkerWorkspace ws;
    ws.ncand = ncand; ws.records = records; ws.label = label; ws.cap = cap;
    ws.ok = hipMemcpyAsync(dict, dict_staged, (size_t)nmarkers * 4, hipMemcpyHostToDevice, s) == hipSuccess;
    if (!ws.ok) return ws;
    const dim3 block(MBLOCK), grid(marker_grid(npix));
    CW_LAUNCH("marker_grey_rows", marker_grey_rows_kernel, dim3((unsigned)(height < 4096 ? height : 4096)), block, 0, s, dev_rgb, width, height, grey, sat);
    CW_LAUNCH("marker_sat_columns", marker_sat_columns_kernel, dim3((unsigned)((width + MBLOCK - 1) / MBLOCK)), block, 0, s, width, height, sat);
    CW_LAUNCH("marker_threshold", marker_threshold_kernel, grid, block, 0, s, grey, sat, width, height, p.window_half, p.threshold_offset, dark, parent, ncand);
    CW_LAUNCH("marker_merge", marker_merge_kernel, grid, block, 0, s, dark, width, height, parent);
    CW_LAUNCH("marker_flatten", marker_flatten_kernel, grid, block, 0, s, parent, npix, label, area, box);
    CW_LAUNCH("marker_stats", marker_stats_kernel, grid, block, 0, s, label, width, npix, area, box);
    CW_LAUNCH("marker_candidates", marker_candidates_kernel, grid, block, 0, s, label, box, width, height, p.min_side, cap, slot, ncand, cand_label, keys);
    CW_LAUNCH("marker_extreme_a", marker_extreme_kernel<0>, grid, block, 0, s, label, slot, width, npix, cap, keys);
    CW_LAUNCH("marker_extreme_c", marker_extreme_kernel<1>, grid, block, 0, s, label, slot, width, npix, cap, keys);
    CW_LAUNCH("marker_extreme_bd", marker_extreme_kernel<2>, grid, block, 0, s, label, slot, width, npix, cap, keys);
    CW_LAUNCH("marker_decode", marker_decode_kernel, dim3(cap < 1024 ? cap : 1024), dim3(64), 0, s, dark, width, height, ncand, cap, cand_label, keys, area,
              dict, nmarkers, p.max_border_errors, p.max_bit_errors, dev_depth, records);
    ws.ok = hipGetLastError() == hipSuccess;
    return ws;
}

void marker_labels_out(const uint32_t *label, size_t npix, int32_t *out, hipStream_t s) {
    CW_LAUNCH("marker_labels_out", marker_labels_out_kernel, dim3(marker_grid(npix)), dim3(MBLOCK), 0, s, label, npix, out);
}

}  // namespace k
}  // namespace cwipc_amd
