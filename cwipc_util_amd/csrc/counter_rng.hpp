// counter_rng.hpp -- the library's stateless random draws (splitmix64 keyed by a 64-bit seed, a tag and a counter) and the per-point
// arithmetic of the two filters that consume them: the noise filter (reference python/cwipc/filters/noise.py:31-50) and the soft
// camera assignment (python/cwipc/filters/simulatecams.py:60-69).  No HIP type: the kernels include it (kernels_floor.hip for its
// shuffle keys, kernels_basic.hip for the two maps), and a host test (tests/test_noise_terms_host.py, through
// tests/abi/noise_terms_host.cpp) compiles the same text with the host C++ compiler and feeds the formulas draws no seed reaches.
//
//   GOLDEN         = 0x9E3779B97F4A7C15
//   base(seed,tag) = splitmix64((seed + tag) mod 2^64)         tag = RNG_TAG_NOISE or RNG_TAG_CAMS
//   draw(b, k)     = splitmix64((b + (k + 1) * GOLDEN) mod 2^64)        k = 0, 1, 2, ...
//   u01(x)         = (double)(x >> 11) * 2^-53                  in [0, 1)
//
// The seed is hashed with the tag, so the two filters do not share a stream on one seed and seeds that differ by a multiple of
// GOLDEN do not give shifted copies of one stream.  tests/scene_model.py is the numpy statement of everything here.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef CWIPC_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_HOST_DEVICE __host__ __device__
#else
#define CWIPC_HOST_DEVICE
#endif
#endif

#ifndef CWIPC_FORCEINLINE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_FORCEINLINE __forceinline__
#else
#define CWIPC_FORCEINLINE inline
#endif
#endif

namespace cwipc_amd {

constexpr unsigned long long RNG_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long RNG_TAG_NOISE = 0x6e6f697365ull;   // "noise"
constexpr unsigned long long RNG_TAG_CAMS = 0x63616d73ull;      // "cams"

// the splitmix64 output function (Steele, Lea, Flood 2014)
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE unsigned long long splitmix64(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE unsigned long long rng_base(unsigned long long seed, unsigned long long tag) { return splitmix64(seed + tag); }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE unsigned long long rng_draw(unsigned long long b, unsigned long long k) { return splitmix64(b + (k + 1ull) * RNG_GOLDEN); }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rng_u01(unsigned long long x) { return (double)(x >> 11) * 0x1.0p-53; }

// One IEEE f64 operation, rounded once.  On the device the round-to-nearest intrinsics (the divide and the root are the correctly
// rounded ones whatever the compiler's fast-math state); on the host the plain operators, compiled with -ffp-contract=off.
#if defined(__HIP_DEVICE_COMPILE__)
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rn_add(double a, double b) { return __dadd_rn(a, b); }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rn_mul(double a, double b) { return __dmul_rn(a, b); }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rn_div(double a, double b) { return __ddiv_rn(a, b); }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rn_sqrt(double a) { return __dsqrt_rn(a); }
#else
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rn_add(double a, double b) { return a + b; }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rn_mul(double a, double b) { return a * b; }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rn_div(double a, double b) { return a / b; }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rn_sqrt(double a) { return std::sqrt(a); }
#endif

// The noise filter's point: u[0..2] -> a vector uniform in the cube (-1, 1)^3, u[3] -> its length as a share of `distance`.
//   v_c = -1 + 2 u_c;  s = (v_0 v_0 + v_1 v_1) + v_2 v_2;  scale = sqrt(s) / u_3;  n_c = (v_c / scale) * distance;
//   out_c = (float)((double)p_c + n_c)
// which is numpy's uniform(-1, 1), linalg.norm(axis=1), rnd_vec / (norm / unif) * distance and `float32 += float64` (evaluated in
// f64, rounded once) on the same draws.  IEEE at the edges, as numpy: u_3 = 0 -> infinite scale -> no noise; s = 0 -> NaN;
// non-finite coordinates propagate.
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void noise_point(const double u[4], double distance, const float p[3], float out[3]) {
    double v[3];
    for (int c = 0; c < 3; c++) v[c] = rn_add(-1.0, rn_mul(2.0, u[c]));
    const double s = rn_add(rn_add(rn_mul(v[0], v[0]), rn_mul(v[1], v[1])), rn_mul(v[2], v[2]));
    const double scale = rn_div(rn_sqrt(s), u[3]);
    for (int c = 0; c < 3; c++) out[c] = (float)rn_add((double)p[c], rn_mul(rn_div(v[c], scale), distance));
}

// point i of a cloud under the noise stream `b` = rng_base(seed, RNG_TAG_NOISE): draws 4 i .. 4 i + 3
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void noise_point_at(unsigned long long b, unsigned long long i, double distance, const float p[3], float out[3]) {
    double u[4];
    for (int j = 0; j < 4; j++) u[j] = rng_u01(rng_draw(b, 4ull * i + (unsigned long long)j));
    noise_point(u, distance, p, out);
}

// The camera of a point under the soft rule.  (vx, vz): the float32-centred position as doubles; dirs: cos, sin per camera.  The dot
// products are the hard rule's (fl(vx cos) first, then one fused multiply-add for vz sin); `first` and `second` are the top two of
// the descending order by (value, camera index) -- of equal dot products the higher index comes first, the reversed stable
// ascending sort.  w = d ** skew (the dot products themselves for skew 1), chance = -w0 + (w1 + w0) u, each step rounded (numpy's
// uniform(low, high) = low + (high - low) u); `first` iff chance < 0, so a NaN chance takes `second`.  ncam >= 2.
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE int soft_camera(int ncam, double vx, double vz, const double *dirs, double skew, double u) {
    int first = 0, second = -1;
    double d_first = 0, d_second = 0;
    for (int c = 0; c < ncam; c++) {
        const double d = fma(vz, dirs[2 * c + 1], rn_mul(vx, dirs[2 * c]));
        if (c == 0) {
            d_first = d;
        } else if (d >= d_first) {
            second = first; d_second = d_first;
            first = c; d_first = d;
        } else if (second < 0 || d >= d_second) {
            second = c; d_second = d;
        }
    }
    const double w0 = skew == 1.0 ? d_first : pow(d_first, skew);
    const double w1 = skew == 1.0 ? d_second : pow(d_second, skew);
    const double chance = rn_add(-w0, rn_mul(rn_add(w1, w0), u));
    return chance < 0 ? first : second;
}

}  // namespace cwipc_amd
