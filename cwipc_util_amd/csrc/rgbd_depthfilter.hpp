// rgbd_depthfilter.hpp -- the arithmetic of the raw entry's depth post-processing (cwipc_hip_rgbd_rig_grab_filtered): the
// step of a line pass of the edge-preserving spatial smoother, the temporal smoother's pixel update and its persistence table.  No HIP
// type: kernels_rgbd.hip includes it for the device, and a host test (tests/test_rgbd_depthfilter_host.py, through
// tests/abi/rgbd_depthfilter_host.cpp) compiles the same text with the host C++ compiler.  tests/rgbd_depthfilter_model.py is its
// numpy / plain-Python statement.
//
// These rules are THIS PROJECT'S OWN definition (hip_ext.h, rule 0): the camera plug-ins that hold the vendors' versions are not in the
// reference tree.  All of it is float64, every operation rounded on its own (rn_* of counter_rng.hpp; the build has
// -ffp-contract=off).  Depth values are in depth units.  oma = 1 - alpha, computed once per call;  q(x) = (uint16) floor(x + 0.5).
//
//   a pass over a line d[0 .. n-1] (rule 0a):         s = (double) d[first]                          running value, 0: none
//     for each further i in pass order:               c = (double) d[i]
//                                                     if d[i] != 0 and s != 0 and |c - s| < delta:   s = (alpha*c) + (oma*s);  d[i] = q(s)
//                                                     else:                                          s = c
//   Starting a pass with s = 0 in FRONT of its first pixel is the same thing: the first pixel then takes the else branch.  That is how
//   the kernels and rgbd_line_pass below do it.  s stays unrounded; a pixel without depth is never filled and resets s.
//   the temporal update of a pixel (rule 0b), c its value after 0a, s its running value (0: none), h its history byte:
//     c != 0:  if s != 0 and |c - s| < delta:  s = (alpha*c) + (oma*s);  out = q(s)     else:  s = c;  out = c
//     c == 0:  out = (s != 0 and persists(mode, h)) ? q(s) : 0                          (s unchanged)
//     h = ((h << 1) | (c != 0)) & 0xff                                                  (persists saw h as it was before)
//   persists(mode, h):  0 never;  1 h == 0xff;  2 popcount(h & 0x07) >= 2;  3 popcount(h & 0x0f) >= 2;  4 popcount(h) >= 2;
//                       5 (h & 0x03) != 0;  6 (h & 0x1f) != 0;  7 h != 0;  8 always
#pragma once

#include <cstddef>
#include <cstdint>

#include "counter_rng.hpp"

namespace cwipc_amd {

constexpr int RGBD_MAX_SPATIAL_MAGNITUDE = 5;
constexpr int RGBD_MAX_PERSISTENCY = 8;

// one stage's numbers: alpha, 1 - alpha and delta
struct RgbdSmoothTerms {
    double alpha, oma, delta;
};

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE RgbdSmoothTerms rgbd_smooth_terms(double alpha, double delta) {
    RgbdSmoothTerms t;
    t.alpha = alpha; t.oma = rn_add(1.0, -alpha); t.delta = delta;
    return t;
}

// q(x): x is in [1, 65535] wherever the rules call it (a convex combination of two depths), so the conversion is in range
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint16_t rgbd_depth_round(double x) { return (uint16_t)(unsigned)__builtin_floor(rn_add(x, 0.5)); }

// do c (a depth, not 0) and the running value s (not 0) blend?
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_depth_near(double c, double s, double delta) {
    const double diff = rn_add(c, -s);
    return (diff < 0.0 ? -diff : diff) < delta;
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rgbd_depth_blend(const RgbdSmoothTerms &t, double c, double s) {
    return rn_add(rn_mul(t.alpha, c), rn_mul(t.oma, s));
}

// The step of a line pass: (s, d) -> (s, d), d the next pixel in pass order.
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void rgbd_line_step(const RgbdSmoothTerms &t, double &s, uint16_t &d) {
    const double c = (double)d;
    const bool blend = d != 0 && s != 0.0 && rgbd_depth_near(c, s, t.delta);
    // (computed whether it is used or not -- c and s lie in 0 .. 65535, so does this -- and chosen: the step has no branch to wait for)
    const double mixed = rgbd_depth_blend(t, c, s);
    s = blend ? mixed : c;
    d = blend ? rgbd_depth_round(mixed) : d;
}

// A whole pass over n pixels `stride` apart, forward from d[0] or backward from d[(n - 1) * stride] (host side: the test program).
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void rgbd_line_pass(const RgbdSmoothTerms &t, uint16_t *d, size_t n, size_t stride, bool backward) {
    double s = 0.0;
    for (size_t i = 0; i < n; i++) rgbd_line_step(t, s, d[(backward ? n - 1 - i : i) * stride]);
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE int rgbd_popcount8(unsigned h) {
    int n = 0;
    for (int bit = 0; bit < 8; bit++) n += (int)((h >> bit) & 1u);
    return n;
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_persists(int mode, unsigned h) {
    h &= 0xffu;
    switch (mode) {
        case 1: return h == 0xffu;
        case 2: return rgbd_popcount8(h & 0x07u) >= 2;
        case 3: return rgbd_popcount8(h & 0x0fu) >= 2;
        case 4: return rgbd_popcount8(h) >= 2;
        case 5: return (h & 0x03u) != 0u;
        case 6: return (h & 0x1fu) != 0u;
        case 7: return h != 0u;
        case 8: return true;
        default: return false;
    }
}

// The temporal update of one pixel: (c, s, h) -> (out, s, h).
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint16_t rgbd_temporal_step(const RgbdSmoothTerms &t, int mode, uint16_t c16, double &s, uint8_t &h) {
    uint16_t out;
    if (c16 != 0) {
        const double c = (double)c16;
        if (s != 0.0 && rgbd_depth_near(c, s, t.delta)) {
            s = rgbd_depth_blend(t, c, s);
            out = rgbd_depth_round(s);
        } else {
            s = c;
            out = c16;
        }
    } else {
        out = (s != 0.0 && rgbd_persists(mode, h)) ? rgbd_depth_round(s) : (uint16_t)0;
    }
    h = (uint8_t)((((unsigned)h << 1) | (c16 != 0 ? 1u : 0u)) & 0xffu);
    return out;
}

}  // namespace cwipc_amd
