// rgbd_terms.hpp -- the per-pixel arithmetic of the RGB-D source (cwipc_hip_from_rgbd): a depth pixel's point in world
// coordinates and the filters a capturer applies while it builds a cloud.  No HIP type: kernels_rgbd.hip includes it for the device,
// rgbd.cpp for the two host mappings (map2d3d, mapcolordepth), and a host test (tests/test_rgbd_terms_host.py, through
// tests/abi/rgbd_terms_host.cpp) compiles the same text with the host C++ compiler.  tests/rgbd_model.py is its numpy statement.
//
// All of it is float64, every operation rounded on its own (rn_* of counter_rng.hpp; the build has -ffp-contract=off).  For pixel
// (u, v) with depth d != 0 of a camera with intrinsics fx, fy, cx, cy, depth_scale and camera -> world matrix m (row-major):
//   z  = (double)d * depth_scale
//   xc = ((double)u - cx) * z / fx           (left to right)          yc = ((double)v - cy) * z / fy
//   X  = ((m00*xc + m01*yc) + m02*z) + m03   (Y, Z alike from rows 1 and 2: the order of kernels_icp.hip)
//   point = (float)X, (float)Y, (float)Z
// The filters, in this order; one whose setting says "off" is skipped:
//   depth range   drop if z < near || z > far                                        off when far <= near
//   height        drop if (double)y < height_min || (double)y > height_max           off when height_min == height_max
//                 (y: the float32 world y)
//   radius        d2 = (float)((double)x*(double)x + (double)z*(double)z) on the float32 world x and z; keep iff d2 < radius*radius,
//                 that product in float32 (reference include/cwipc_util/internal/capturers.hpp:210-213)      off when radius <= 0
//   green screen  drop iff 60 <= hue <= 130, hue the reference's integer one (rgbToHsv, capturers.hpp:223-253)  off when green == 0
// The depth-range and height rules and their "off" conventions are this project's own; the reference's are in camera plug-ins.
//
// The green screen.  The reference's isNotGreen (:256-275) also looks at s and v inside the hue window and edits r and b there.  hue is
// only ever non-zero when v != 0 and s != 0, s and v are unsigned char, and they are compared with 0.15, 0.4 and 0.3: inside the
// window both conditions hold, every point there is dropped and the edited colours reach no output.  The hue test alone decides;
// the host test runs the full restatement over all 2^24 colours against it.
#pragma once

#include "counter_rng.hpp"

namespace cwipc_amd {

struct RgbdCamTerms {
    double fx, fy, cx, cy, depth_scale;
    double m[12];   // rows 0-2 of the camera -> world matrix
};

struct RgbdFilterTerms {
    double near_z, far_z;
    double height_min, height_max;
    float radius;
    int green;
};

constexpr unsigned RGBD_DEPTH_RANGE = 1u, RGBD_HEIGHT = 2u, RGBD_RADIUS = 4u, RGBD_GREEN = 8u;

// which filters are on
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE unsigned rgbd_active(const RgbdFilterTerms &f) {
    unsigned a = 0;
    if (!(f.far_z <= f.near_z)) a |= RGBD_DEPTH_RANGE;
    if (!(f.height_min == f.height_max)) a |= RGBD_HEIGHT;
    if (!(f.radius <= 0.0f)) a |= RGBD_RADIUS;
    if (f.green != 0) a |= RGBD_GREEN;
    return a;
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rgbd_z(unsigned d, double depth_scale) { return rn_mul((double)d, depth_scale); }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rgbd_xc(const RgbdCamTerms &c, int u, double z) { return rn_div(rn_mul(rn_add((double)u, -c.cx), z), c.fx); }
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rgbd_yc(const RgbdCamTerms &c, int v, double z) { return rn_div(rn_mul(rn_add((double)v, -c.cy), z), c.fy); }
// one world coordinate: row 0, 1 or 2 of the matrix
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE float rgbd_world(const RgbdCamTerms &c, int row, double xc, double yc, double z) {
    const double *m = c.m + 4 * row;
    return (float)rn_add(rn_add(rn_add(rn_mul(m[0], xc), rn_mul(m[1], yc)), rn_mul(m[2], z)), m[3]);
}

// the point of pixel (u, v) with depth d (the caller has seen that d != 0; the arithmetic is defined for every d)
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void rgbd_point(const RgbdCamTerms &c, int u, int v, unsigned d, float out[3]) {
    const double z = rgbd_z(d, c.depth_scale), xc = rgbd_xc(c, u, z), yc = rgbd_yc(c, v, z);
    for (int row = 0; row < 3; row++) out[row] = rgbd_world(c, row, xc, yc, z);
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_in_radius(float x, float z, float radius) {
    const float d2 = (float)rn_add(rn_mul((double)x, (double)x), rn_mul((double)z, (double)z));
    return d2 < radius * radius;
}

// the reference's hue: unsigned char fields, C integer division (towards zero), the result stored into an unsigned char
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE unsigned rgbd_hue(unsigned r, unsigned g, unsigned b) {
    const int ri = (int)r, gi = (int)g, bi = (int)b;
    const int mn = ri < gi ? (ri < bi ? ri : bi) : (gi < bi ? gi : bi);
    const int mx = ri > gi ? (ri > bi ? ri : bi) : (gi > bi ? gi : bi);
    if (mx == 0) return 0u;
    if ((unsigned char)(255 * (long)(mx - mn) / mx) == 0) return 0u;
    int h;
    if (mx == ri) h = 0 + 43 * (gi - bi) / (mx - mn);
    else if (mx == gi) h = 85 + 43 * (bi - ri) / (mx - mn);
    else h = 171 + 43 * (ri - gi) / (mx - mn);
    return (unsigned)(unsigned char)h;
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_not_green(unsigned r, unsigned g, unsigned b) {
    const unsigned h = rgbd_hue(r, g, b);
    return !(h >= 60u && h <= 130u);
}

// Does pixel (u, v) with depth d give a point?  `active`: rgbd_active(f).  colour() -> r | g << 8 | b << 16, asked for only when the
// green screen is on and nothing else has dropped the pixel; of the point only the coordinates an active filter looks at are computed.
template <class Colour>
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_keep(const RgbdCamTerms &c, const RgbdFilterTerms &f, unsigned active, int u, int v, unsigned d, Colour colour) {
    if (d == 0u) return false;
    const double z = rgbd_z(d, c.depth_scale);
    if ((active & RGBD_DEPTH_RANGE) && (z < f.near_z || z > f.far_z)) return false;
    if (active & (RGBD_HEIGHT | RGBD_RADIUS)) {
        const double xc = rgbd_xc(c, u, z), yc = rgbd_yc(c, v, z);
        if (active & RGBD_HEIGHT) {
            const double y = (double)rgbd_world(c, 1, xc, yc, z);
            if (y < f.height_min || y > f.height_max) return false;
        }
        if ((active & RGBD_RADIUS) && !rgbd_in_radius(rgbd_world(c, 0, xc, yc, z), rgbd_world(c, 2, xc, yc, z), f.radius)) return false;
    }
    if (active & RGBD_GREEN) {
        const unsigned w = colour();
        if (!rgbd_not_green(w & 255u, (w >> 8) & 255u, (w >> 16) & 255u)) return false;
    }
    return true;
}

}  // namespace cwipc_amd
