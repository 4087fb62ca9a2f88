// voxel_anchor.hpp -- the host arithmetic of the voxel-grid downsample: the octree's anchor box and leaf-face thresholds, and how a
// cloud's wave steps are dealt to the accumulate kernels' workgroups.  Numbers in, numbers out, no HIP type or call: the host C++
// compiler alone compiles it (tests/test_voxel_anchor_host.py, through tests/abi/voxel_anchor_host.cpp, checks the definitions).
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include "voxel_common.hpp"
namespace cwipc_amd {
namespace {

// ---------------------------------------------------------------------------
// host: anchor and face thresholds  [PCL upstream octree_pointcloud.hpp]
// ---------------------------------------------------------------------------
// Octree box after the first point: adoptBoundingBoxToPoint's "octree is empty" branch followed
// by getKeyBitSize().
void first_box(const double p[3], double res, double mn[3], double mx[3], int &depth) {
    const double eps = (double)FLT_EPSILON;
    unsigned max_key = 0;
    for (int a = 0; a < 3; a++) {
        mn[a] = p[a] - res / 2;
        mx[a] = p[a] + res / 2;
        unsigned mk = (unsigned)ceil((mx[a] - mn[a] - eps) / res);
        max_key = mk > max_key ? mk : max_key;
    }
    unsigned max_voxels = max_key > 2 ? max_key : 2;
    double d = ceil(log2((double)max_voxels) - eps);
    d = d > 32 ? 32 : (d < 0 ? 0 : d);
    depth = (int)d;
    double side = (double)(1u << depth) * res;
    for (int a = 0; a < 3; a++) {
        double oversize = (side - (mx[a] - mn[a])) / 2.0;
        if (oversize > eps) {
            mn[a] -= oversize;
            mx[a] += oversize;
        }
    }
}

// Smallest float for which a monotone predicate (false ... false true ... true over the ordered floats) holds, searched
// outwards from a guess: doubling steps until the answer is bracketed, then bisection.  The guess is a few float steps
// off as a rule (a dozen evaluations); it may be ~1e28 steps off near zero, where the double sum p - min absorbs
// them all (a face through a first point with a coordinate of -5e-17: a cloud rotated by 270 degrees) -- hence no
// fixed-width search, and hence not 32 bisection steps from the ends of the float line for every one of 768 table
// entries either (120 us per call for a cloud whose anchor is new, as every tile of a capture is).
template <class Pred>
float first_float_where(const Pred &passes, float guess) {
    const auto to_ord = [](float f) { int32_t b; memcpy(&b, &f, 4); return b >= 0 ? (int64_t)b : -(int64_t)(b & 0x7fffffff); };
    const auto from_ord = [](int64_t o) { int32_t b = o >= 0 ? (int32_t)o : (int32_t)(0x80000000u | (uint32_t)(-o)); float f; memcpy(&f, &b, 4); return f; };
    const int64_t lowest = to_ord(-FLT_MAX), highest = to_ord(FLT_MAX);
    if (!(guess >= -FLT_MAX && guess <= FLT_MAX)) guess = 0.f;
    int64_t lo, hi;   // invariant at the end: lo fails, hi passes
    const int64_t g = to_ord(guess);
    if (passes(from_ord(g))) {
        hi = g;
        int64_t step = 1;
        for (;;) {
            lo = hi - step;
            if (lo <= lowest) { lo = lowest; if (passes(from_ord(lo))) return -FLT_MAX; break; }
            if (!passes(from_ord(lo))) break;
            hi = lo;
            step *= 2;
        }
    } else {
        lo = g;
        int64_t step = 1;
        for (;;) {
            hi = lo + step;
            if (hi >= highest) { hi = highest; if (!passes(from_ord(hi))) return INFINITY; break; }
            if (passes(from_ord(hi))) break;
            lo = hi;
            step *= 2;
        }
    }
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (passes(from_ord(mid))) hi = mid; else lo = mid;
    }
    return from_ord(hi);
}

// The octree key of a coordinate, floor((p - min) / resolution) in double (genOctreeKeyforPoint), is monotone in p:
// "key >= m" is a threshold test p >= T(m).  Smallest float that passes.
float leaf_threshold(double mn0, double res, int m) {
    const double md = (double)m;
    return first_float_where([&](float p) { return floor(((double)p - mn0) / res) >= md; }, (float)(mn0 + md * res));
}

// Smallest float whose voxel index floor(fl(p * inv_leaf)) exceeds `voxel` (fp32 product, as the kernels compute it).
float voxel_upper_bound(float inv_leaf, int voxel) {
    return first_float_where([&](float p) { return floorf(p * inv_leaf) > (float)voxel; }, (float)(((double)voxel + 1.0) / (double)inv_leaf));
}

// The face table of one anchor: per axis and face the threshold T, the voxel tf it cuts and where the voxel above begins (Tv).
void fill_face_table(const double mn0[3], double res, const int face_base[3], float inv_leaf, uint32_t faces_host[FACE_TABLE_WORDS]) {
    for (int a = 0; a < 3; a++) {
        for (int i = 0; i < FACES; i++) {
            const float T = leaf_threshold(mn0[a], res, face_base[a] + i);
            // the voxel the face cuts (the fp32 product and floor of the kernels), and where the voxel above it begins
            const float g = floorf(T * inv_leaf);
            const bool sane = std::isfinite(T) && fabsf(g) < 1.0e9f;
            const int tf = sane ? (int)g : (T > 0 ? INT32_MAX : INT32_MIN);
            const float Tv = sane ? voxel_upper_bound(inv_leaf, tf) : T;
            memcpy(&faces_host[FT_T + a * FACES + i], &T, 4);
            memcpy(&faces_host[FT_TV + a * FACES + i], &Tv, 4);
            memcpy(&faces_host[FT_TF + a * FACES + i], &tf, 4);
        }
    }
}

// ---------------------------------------------------------------------------
// host: range plans
// ---------------------------------------------------------------------------
// The general accumulate kernel's wave ranges on `cus` compute units, workgroups 2^shrink times smaller than one per CU:
// one persistent workgroup per CU; short clouds get fewer so that every wave has at least one step,
// very large clouds get more (sequential) workgroups: the packed table needs < 65536 points per workgroup
inline size_t general_plan_waves(size_t n, int cus, int shrink) {
    size_t nwaves = ((size_t)cus * K1_WAVES) << shrink;
    const size_t steps_total = (n + WAVE_STEP - 1) / WAVE_STEP;
    if (nwaves > steps_total) nwaves = ((steps_total + K1_WAVES - 1) / K1_WAVES) * K1_WAVES;
    const size_t min_waves = (n + MAX_POINTS_PER_WAVE - 1) / MAX_POINTS_PER_WAVE;
    if (nwaves < min_waves) nwaves = ((min_waves + K1_WAVES - 1) / K1_WAVES) * K1_WAVES;
    return nwaves;
}
// ... and the points of each wave range (a multiple of WAVE_STEP)
inline size_t general_plan_per_wave(size_t n, size_t nwaves) { return (((n + nwaves - 1) / nwaves + WAVE_STEP - 1) / WAVE_STEP) * WAVE_STEP; }

// The fast accumulate kernel's workgroup ranges: `blocks` of them, `per_wg` points the longest; base_q / inc_q != 0: of growing
// lengths (range_first_step).  `stagger`: per cent (CWIPC_K1_STAGGER).
struct FastPlan { uint32_t blocks, per_wg, base_q, inc_q; };
inline FastPlan fast_plan(size_t n, int cus, int stagger_knob) {
    const size_t steps_total = (n + WAVE_STEP - 1) / WAVE_STEP;
    // The workgroups' ranges: the cloud's steps dealt evenly over the CUs the grid may use (a workgroup's waves share its
    // range step by step, so a range need not be a multiple of sixteen steps): a 300 k-point cloud gets 235 workgroups
    // of 5 steps, five busy waves each, instead of 74 workgroups whose sixteen waves queue up on four SIMDs.
    const size_t wg_steps = std::min<size_t>(std::max<size_t>((steps_total + cus - 1) / cus, 1), MAX_POINTS_PER_WAVE * K1_WAVES / WAVE_STEP);
    FastPlan plan{(uint32_t)((steps_total + wg_steps - 1) / wg_steps), (uint32_t)(wg_steps * WAVE_STEP), 0u, 0u};
    const uint32_t fast_blocks = plan.blocks;
    // r4: the ranges' lengths grow linearly with the workgroup's number, from (1 - p %) to (1 + p %) of the mean, so that the
    // workgroups reach their flush one after the other: the memory side takes ~10 us for all the flushes' atomics (112 k
    // entries x seven), during which nothing streams when 248 workgroups arrive within two microseconds.  The longest range
    // sets the kernel's end now (a workgroup's streaming time goes with its length: the vector port, not the memory, bounds it),
    // so only part of those 10 us comes back: 53.9-54.4 -> 51.2-51.9 us alone at p = 20-25, 15 does nothing, 30-40 lose it again;
    // a call in a stream is what it was (47-48 us: there the next kernel's workgroups fill the gaps anyway), call-then-count
    // 66.0 -> 64.2 (profiles/r04_k1_stagger.txt).  CWIPC_K1_STAGGER=p overrides (0: equal ranges, rounds 1-3).  Only for
    // ranges of 24 steps or more (clouds from 1.5 M points): a short range is mostly set-up and flush.
    if (stagger_knob > 0 && stagger_knob < 60 && fast_blocks >= 64 && steps_total >= (size_t)24 * fast_blocks && n < ((size_t)1 << 31)) {
        const double mean_q = (double)steps_total * 1024.0 / (double)fast_blocks, s_frac = stagger_knob / 100.0;
        const size_t max_steps = MAX_POINTS_PER_WAVE * K1_WAVES / WAVE_STEP;
        uint32_t inc = (uint32_t)ceil(2.0 * s_frac * mean_q / (double)(fast_blocks - 1));
        uint32_t base = (uint32_t)ceil(mean_q * (1.0 - s_frac));
        while (range_first_step(fast_blocks, base, inc) < steps_total) base++;
        const size_t longest = (size_t)((base + (unsigned long long)(fast_blocks - 1) * inc + 2047) >> 10);
        if (base >= 1024 && longest <= max_steps) {
            plan.base_q = base; plan.inc_q = inc;
            plan.per_wg = (uint32_t)(longest * WAVE_STEP);
        }
    }
    return plan;
}

}  // namespace
}  // namespace cwipc_amd
