// rgbd_decimate.hpp -- the arithmetic of the raw entry's depth decimation (cwipc_hip_rgbd_rig_create_decimated) and hole filling
// (cwipc_hip_rgbd_rig_grab_filled), DESIGN 3.23: the derived sensor of a decimated rig, the value of a decimated pixel from the k * k
// source pixels of its block, the fill operator of mode 1 and the pick of modes 2 and 3.  No HIP type: kernels_rgbd.hip includes it for
// the device, rgbd_stage.hpp for the derived sensors, and a host test (tests/test_rgbd_decimate_host.py, through
// tests/abi/rgbd_decimate_host.cpp) compiles the same text with the host C++ compiler.  tests/rgbd_decimate_model.py is its numpy
// statement.
//
// These rules are THIS PROJECT'S OWN definition (hip_ext.h, RULE D and rule 0c): the camera plug-ins that hold the vendors' versions
// are not in the reference tree.  Arithmetic is float64, every operation rounded on its own (rn_* of counter_rng.hpp; the build has
// -ffp-contract=off);  q(x) = (uint16) floor(x + 0.5)  as in rule 0.
//
//   RULE D, decimation k = 1 .. 8 of a sensor W x H, fx fy cx cy:
//     W' = W div k;  H' = H div k          source columns from k*W' and rows from k*H' on are never read
//     fx' = fx / k;  fy' = fy / k
//     cx' = (cx - (k - 1) * 0.5) / k;  cy' alike      decimated pixel U sits at the centre of source pixels kU .. kU + k - 1
//     everything else of the sensor is unchanged.  k == 1: the sensor itself, bit for bit (x - 0 and x / 1 are exact).
//   the value of decimated pixel (U, V), n the number of NON-ZERO values among the k * k source pixels (kU + i, kV + j), 0 <= i, j < k:
//     n == 0:       0
//     k = 2, 3:     the LOWER MEDIAN: the non-zero values sorted ascending, a[(n - 1) div 2]
//     k = 4 .. 8:   q((double) sum / (double) n), sum the exact integer sum of the non-zero values (at most 64 * 65535: 32 bits)
//     n > 0 gives a value in 1 .. 65535: no clamp is part of the rule.
//   rule 0c, hole filling, mode 1 .. 3, per camera on the rig's grid, after 0b and before erosion.  A pixel with depth is never changed.
//     mode 1:  a pixel without depth takes the value of the nearest pixel WITH depth to its left in its row; none: it stays 0.
//              out[i] = op(out[i - 1], d[i]) with op(a, b) = b != 0 ? b : a, out[-1] = 0.  op is associative (0 its identity): a scan.
//     mode 2:  a pixel without depth takes the LARGEST non-zero value among its up to eight neighbours inside the image, read from
//              the stage's INPUT (not in place: nothing propagates, no order); none: it stays 0.
//     mode 3:  the same with the SMALLEST non-zero value.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rgbd_depthfilter.hpp"

namespace cwipc_amd {

constexpr int RGBD_MAX_DECIMATION = 8;
constexpr int RGBD_MAX_HOLEFILL = 3;

// the depth side of a sensor on the decimated grid
struct RgbdGrid {
    int width, height;
    double fx, fy, cx, cy;
};

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rgbd_decimated_centre(double c, int k) {
    return rn_div(rn_add(c, -rn_mul((double)(k - 1), 0.5)), (double)k);
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE RgbdGrid rgbd_derived_grid(int width, int height, double fx, double fy, double cx, double cy, int k) {
    RgbdGrid g;
    g.width = width / k; g.height = height / k;
    g.fx = rn_div(fx, (double)k); g.fy = rn_div(fy, (double)k);
    g.cx = rgbd_decimated_centre(cx, k); g.cy = rgbd_decimated_centre(cy, k);
    return g;
}

// The lower median of the non-zero values among a[0 .. N-1] (n of them, n > 0).  A pixel without depth is handed in as 0x10000, above
// every depth, so the n values with depth are the first n after sorting.  The loops have constant bounds: unrolled, a stays in
// registers (a bubble network, 36 compare-exchanges for N = 9), and the pick is a chain of selects.
template <int N>
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint16_t rgbd_lower_median(uint32_t (&a)[N], int n) {
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
#pragma unroll
        for (int j = 0; j < N - 1 - i; j++) {
            const uint32_t lo = a[j] < a[j + 1] ? a[j] : a[j + 1], hi = a[j] < a[j + 1] ? a[j + 1] : a[j];
            a[j] = lo; a[j + 1] = hi;
        }
    }
    const int at = (n - 1) / 2;
    uint32_t rv = a[0];
#pragma unroll
    for (int i = 1; i <= (N - 1) / 2; i++) rv = at == i ? a[i] : rv;
    return (uint16_t)rv;
}

// q(sum / n), n > 0
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint16_t rgbd_block_mean(uint32_t sum, uint32_t n) { return rgbd_depth_round(rn_div((double)sum, (double)n)); }

// The value of a block from its K * K values, in any order.
template <int K>
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint16_t rgbd_block_value(const uint16_t (&v)[K * K]) {
    static_assert(K >= 2 && K <= RGBD_MAX_DECIMATION, "decimation 2 .. 8");
    int n = 0;
    if constexpr (K <= 3) {
        uint32_t a[K * K];
#pragma unroll
        for (int i = 0; i < K * K; i++) {
            a[i] = v[i] != 0 ? (uint32_t)v[i] : 0x10000u;
            n += v[i] != 0 ? 1 : 0;
        }
        return n == 0 ? (uint16_t)0 : rgbd_lower_median<K * K>(a, n);
    } else {
        uint32_t sum = 0;
#pragma unroll
        for (int i = 0; i < K * K; i++) {
            sum += v[i];
            n += v[i] != 0 ? 1 : 0;
        }
        return n == 0 ? (uint16_t)0 : rgbd_block_mean(sum, (uint32_t)n);
    }
}

// Decimated pixel (U, V) of a source image `width` wide (host side: rgbd_rig.cpp has no use for it, the test program has).
template <int K>
inline uint16_t rgbd_decimated_pixel(const uint16_t *src, size_t width, size_t U, size_t V) {
    uint16_t v[K * K];
    for (int j = 0; j < K; j++)
        for (int i = 0; i < K; i++) v[j * K + i] = src[((size_t)K * V + (size_t)j) * width + (size_t)K * U + (size_t)i];
    return rgbd_block_value<K>(v);
}

// A whole image (host side): dst has (width div k) * (height div k) pixels.  false: k is not 2 .. 8.
inline bool rgbd_decimate_image(const uint16_t *src, size_t width, size_t height, int k, uint16_t *dst) {
    const size_t w = width / (size_t)(k > 0 ? k : 1), h = height / (size_t)(k > 0 ? k : 1);
    for (size_t V = 0; V < h; V++)
        for (size_t U = 0; U < w; U++) {
            uint16_t &out = dst[V * w + U];
            switch (k) {
                case 2: out = rgbd_decimated_pixel<2>(src, width, U, V); break;
                case 3: out = rgbd_decimated_pixel<3>(src, width, U, V); break;
                case 4: out = rgbd_decimated_pixel<4>(src, width, U, V); break;
                case 5: out = rgbd_decimated_pixel<5>(src, width, U, V); break;
                case 6: out = rgbd_decimated_pixel<6>(src, width, U, V); break;
                case 7: out = rgbd_decimated_pixel<7>(src, width, U, V); break;
                case 8: out = rgbd_decimated_pixel<8>(src, width, U, V); break;
                default: return false;
            }
        }
    return true;
}

// mode 1's operator: the value to the left, a, and the pixel, b
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint16_t rgbd_fill_op(uint16_t a, uint16_t b) { return b != 0 ? b : a; }

// modes 2 and 3: the pixel's new value from the 3 x 3 values around it, row-major, n[4] the pixel itself, 0 for a neighbour outside
// the image
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint16_t rgbd_fill_pick(int mode, const uint16_t (&n)[9]) {
    if (n[4] != 0) return n[4];
    uint32_t best = mode == 2 ? 0u : 0x10000u;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint32_t v = n[i];
        const bool better = v != 0u && (mode == 2 ? v > best : v < best);
        best = better ? v : best;
    }
    return best == 0x10000u ? (uint16_t)0 : (uint16_t)best;
}

// Rule 0c on a whole image (host side: the test program): in -> out, two different images of width * height pixels.
inline void rgbd_holefill_image(int mode, const uint16_t *in, size_t width, size_t height, uint16_t *out) {
    for (size_t v = 0; v < height; v++) {
        uint16_t run = 0;
        for (size_t u = 0; u < width; u++) {
            if (mode == 1) {
                run = rgbd_fill_op(run, in[v * width + u]);
                out[v * width + u] = run;
            } else if (mode == 2 || mode == 3) {
                uint16_t n[9];
                for (int dv = -1; dv <= 1; dv++)
                    for (int du = -1; du <= 1; du++) {
                        const ptrdiff_t y = (ptrdiff_t)v + dv, x = (ptrdiff_t)u + du;
                        const bool inside = y >= 0 && x >= 0 && y < (ptrdiff_t)height && x < (ptrdiff_t)width;
                        n[(dv + 1) * 3 + du + 1] = inside ? in[(size_t)y * width + (size_t)x] : (uint16_t)0;
                    }
                out[v * width + u] = rgbd_fill_pick(mode, n);
            } else {
                out[v * width + u] = in[v * width + u];
            }
        }
    }
}

}  // namespace cwipc_amd
