// quality_terms.hpp -- the arithmetic of RULE Q (include/cwipc_util_amd/hip_ext.h): what a matched pair of cwipc_hip_distortion
// contributes to the sums.  No HIP type: the sums kernel (DistortionPair of kernels_icp.hip) includes it, and a host test
// (tests/test_quality_terms_host.py, through tests/abi/quality_terms_host.cpp) compiles the same text with the host C++ compiler and
// checks it bit for bit against the numpy model (tests/quality_model.py).  Every operation is rounded on its own, in f64
// (-ffp-contract=off); the order of the operations below IS the contract.
//
// The measures are those of MPEG's pc_error (point-to-point D1, point-to-plane D2, colour in BT.709 YUV); the rule itself -- which
// point is matched, which normal a pair has -- is this project's own and is stated in hip_ext.h.
#pragma once

#include <cstdint>

#ifndef CWIPC_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_HOST_DEVICE __host__ __device__
#else
#define CWIPC_HOST_DEVICE
#endif
#endif

namespace cwipc_amd {

constexpr int QUALITY_NTERM = 10;   // 1 | 1 or 0: the pair has a normal | d2 | r^2 | dR^2, dG^2, dB^2 | dY^2, dU^2, dV^2

// The 10 terms of a matched pair: p the source point, q the matched reference point, m the pair's normal (not read when the pair
// has none), all (double) of float32; the two packed colour words (r | g << 8 | b << 16 | tile << 24), the source's and the
// reference's; d2 the pair's squared distance, as the search found it.
CWIPC_HOST_DEVICE inline void quality_pair_terms(const double p[3], const double q[3], const double m[3], bool has_normal, uint32_t source_rgbt,
                                                 uint32_t reference_rgbt, double d2, double out[QUALITY_NTERM]) {
    out[0] = 1.0;
    out[2] = d2;
    if (has_normal) {
        const double e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
        const double r = (e[0] * m[0] + e[1] * m[1]) + e[2] * m[2];
        out[1] = 1.0;
        out[3] = r * r;
    } else {
        out[1] = 0.0;
        out[3] = 0.0;
    }
    // the source's colour byte minus the reference's: integers in -255 .. 255
    const double dR = (double)((int)(source_rgbt & 255u) - (int)(reference_rgbt & 255u));
    const double dG = (double)((int)((source_rgbt >> 8) & 255u) - (int)((reference_rgbt >> 8) & 255u));
    const double dB = (double)((int)((source_rgbt >> 16) & 255u) - (int)((reference_rgbt >> 16) & 255u));
    // BT.709, as in pc_error (the offsets of 128 cancel in a difference)
    const double dY = (0.2126 * dR + 0.7152 * dG) + 0.0722 * dB;
    const double dU = (-0.1146 * dR - 0.3854 * dG) + 0.5 * dB;
    const double dV = (0.5 * dR - 0.4542 * dG) - 0.0458 * dB;
    out[4] = dR * dR;
    out[5] = dG * dG;
    out[6] = dB * dB;
    out[7] = dY * dY;
    out[8] = dU * dU;
    out[9] = dV * dV;
}

}  // namespace cwipc_amd
