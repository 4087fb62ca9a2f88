// rgbd_lens.hpp -- the arithmetic of the RGB-D source's RAW entry (cwipc_hip_rgbd_rig_grab): lens distortion, the depth
// camera's ray table, the projection of a depth pixel's point into the colour camera, and the erosion rule.  No HIP type:
// kernels_rgbd.hip includes it for the device, rgbd_rig.cpp for the ray tables and the host mappings, and a host test
// (tests/test_rgbd_lens_host.py, through tests/abi/rgbd_lens_host.cpp) compiles the same text with the host C++ compiler.
// tests/rgbd_lens_model.py is its numpy statement.  rgbd_terms.hpp (the world point and the four filters) is used as it is.
//
// These rules are THIS PROJECT'S OWN definition: the camera plug-ins that hold the reference's versions are not in the reference tree.
// All of it is float64, every operation rounded on its own (rn_* of counter_rng.hpp; the build has -ffp-contract=off); every
// parenthesis below is part of the contract.  coeffs = k1 k2 p1 p2 k3 k4 k5 k6, OpenCV's rational model.
//
//   distort(x, y):
//     xx = x*x;  yy = y*y;  r2 = xx + yy
//     num = 1 + r2*(k1 + r2*(k2 + r2*k3));  den = 1 + r2*(k4 + r2*(k5 + r2*k6));  rad = num / den
//     a1 = (2*x)*y;  a2 = r2 + 2*xx;  a3 = r2 + 2*yy
//     x' = (x*rad + p1*a1) + p2*a2;         y' = (y*rad + p1*a3) + p2*a1
//   its Jacobian J (for Newton's method; dn = k1 + r2*(2*k2 + r2*(3*k3)), dd = k4 + r2*(2*k5 + r2*(3*k6))):
//     g   = (dn*den - num*dd) / (den*den)                                   (d rad / d r2)
//     j00 = ((rad + (2*xx)*g) + (2*p1)*y) + (6*p2)*x      j01 = (((2*x)*y)*g + (2*p1)*x) + (2*p2)*y
//     j10 = j01                                           j11 = ((rad + (2*yy)*g) + (6*p1)*y) + (2*p2)*x
//     det = j00*j11 - j01*j10
//   ray(u, v) of a depth camera (fx fy cx cy, coeffs):  xd = (u - cx) / fx;  yd = (v - cy) / fy
//     all eight coefficients zero: (xd, yd).  Otherwise Newton's method from (x, y) = (xd, yd):
//       repeat: (x', y') = distort(x, y);  ex = x' - xd;  ey = y' - yd
//               if |ex| < 1e-12 and |ey| < 1e-12: the entry is (x, y) if det(x, y) > 0, else (NaN, NaN); stop
//               if 20 steps have been taken: (NaN, NaN); stop
//               x = x - (j11*ex - j01*ey) / det;   y = y - (j00*ey - j10*ex) / det
//     (NaN, NaN): the pixel has no ray and gives no point.  A NaN anywhere fails both comparisons and ends as (NaN, NaN).
//   the point of pixel (u, v), depth d:  z = d * depth_scale;  xc = xn*z;  yc = yn*z with (xn, yn) = ray(u, v), then rgbd_world.
//     EXCEPTION: a sensor whose eight depth coefficients are all zero uses rgbd_xc / rgbd_yc of rgbd_terms.hpp instead, so that the
//     raw entry degenerates to cwipc_hip_from_rgbd bit for bit.
//   the colour pixel of that point (m = depth_to_colour, rows 0-2, row-major; fxc fyc cxc cyc, coeffs of the colour camera, Wc x Hc):
//     Px = ((m00*xc + m01*yc) + m02*z) + m03,  Py and Pz alike
//     Pz <= 0, or Pz not finite: none.  (x', y') = distort(Px / Pz, Py / Pz) with the colour coefficients (always, also all zero)
//     uc = floor((fxc*x' + cxc) + 0.5);  vc = floor((fyc*y' + cyc) + 0.5)
//     none unless 0 <= uc < Wc and 0 <= vc < Hc, tested ON THE DOUBLES (a NaN fails); else the pixel (int)uc, (int)vc.
//   Nearest pixel; occlusion between the two sensors is NOT modelled unless asked for: without it a point the colour camera cannot
//   see takes the colour of whatever is in front of it there.
//   occlusion (splat 0 .. 8 colour pixels, margin >= 0 metres; cwipc_hip_rgbd_rig_grab_occluded), per camera:
//     candidate: a depth pixel that has depth after erosion and a colour pixel (uc, vc) by the rule above (so a ray, and Pz finite, > 0)
//     Zmin(a, b) = the minimum of Pz(q) over the candidates q with |uc(q) - a| <= splat and |vc(q) - b| <= splat, (a, b) inside the image
//     candidate p is occluded iff Zmin(uc(p), vc(p)) < Pz(p) - margin: one subtraction, a strict comparison.  It then is a pixel
//     without a colour.  A positive finite double's bits order as an unsigned 64-bit integer does (Pz > 0: neither zero occurs), so the
//     minimum is an unsigned minimum of rgbd_depth_key and does not depend on the order it is taken in; all ones is above every key.
//     Nor does it depend on whether a candidate's key is written to its whole square and read at one cell, or written to its own
//     cell and read over the square: the kernels do the latter.
//   erosion (ex, ey): a pixel keeps its depth iff no pixel (u + du, v + dv), |du| <= ex, |dv| <= ey, INSIDE the image has depth 0.
#pragma once

#include "rgbd_terms.hpp"

namespace cwipc_amd {

struct RgbdLens {
    double k1, k2, p1, p2, k3, k4, k5, k6;
};

// the colour side of a sensor: where a point in depth-camera coordinates lands in the colour image
struct RgbdColourTerms {
    double fx, fy, cx, cy;
    RgbdLens lens;
    double m[12];   // rows 0-2 of depth_to_colour
    int width, height;
};

constexpr int RGBD_NEWTON_STEPS = 20;
constexpr double RGBD_NEWTON_EPS = 1e-12;
constexpr int RGBD_MAX_EROSION = 32;

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_lens_is_pinhole(const RgbdLens &l) {
    return l.k1 == 0.0 && l.k2 == 0.0 && l.p1 == 0.0 && l.p2 == 0.0 && l.k3 == 0.0 && l.k4 == 0.0 && l.k5 == 0.0 && l.k6 == 0.0;
}

// what distort and its Jacobian share
struct RgbdRadial {
    double xx, yy, r2, num, den, rad;
};

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE RgbdRadial rgbd_radial(const RgbdLens &l, double x, double y) {
    RgbdRadial r;
    r.xx = rn_mul(x, x);
    r.yy = rn_mul(y, y);
    r.r2 = rn_add(r.xx, r.yy);
    r.num = rn_add(1.0, rn_mul(r.r2, rn_add(l.k1, rn_mul(r.r2, rn_add(l.k2, rn_mul(r.r2, l.k3))))));
    r.den = rn_add(1.0, rn_mul(r.r2, rn_add(l.k4, rn_mul(r.r2, rn_add(l.k5, rn_mul(r.r2, l.k6))))));
    r.rad = rn_div(r.num, r.den);
    return r;
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void rgbd_distort_with(const RgbdLens &l, const RgbdRadial &r, double x, double y, double out[2]) {
    const double a1 = rn_mul(rn_mul(2.0, x), y);
    const double a2 = rn_add(r.r2, rn_mul(2.0, r.xx));
    const double a3 = rn_add(r.r2, rn_mul(2.0, r.yy));
    out[0] = rn_add(rn_add(rn_mul(x, r.rad), rn_mul(l.p1, a1)), rn_mul(l.p2, a2));
    out[1] = rn_add(rn_add(rn_mul(y, r.rad), rn_mul(l.p1, a3)), rn_mul(l.p2, a1));
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void rgbd_distort(const RgbdLens &l, double x, double y, double out[2]) {
    rgbd_distort_with(l, rgbd_radial(l, x, y), x, y, out);
}

// j = j00 j01 j10 j11; returns det
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rgbd_jacobian(const RgbdLens &l, const RgbdRadial &r, double x, double y, double j[4]) {
    const double dn = rn_add(l.k1, rn_mul(r.r2, rn_add(rn_mul(2.0, l.k2), rn_mul(r.r2, rn_mul(3.0, l.k3)))));
    const double dd = rn_add(l.k4, rn_mul(r.r2, rn_add(rn_mul(2.0, l.k5), rn_mul(r.r2, rn_mul(3.0, l.k6)))));
    const double g = rn_div(rn_add(rn_mul(dn, r.den), -rn_mul(r.num, dd)), rn_mul(r.den, r.den));
    j[0] = rn_add(rn_add(rn_add(r.rad, rn_mul(rn_mul(2.0, r.xx), g)), rn_mul(rn_mul(2.0, l.p1), y)), rn_mul(rn_mul(6.0, l.p2), x));
    j[1] = rn_add(rn_add(rn_mul(rn_mul(rn_mul(2.0, x), y), g), rn_mul(rn_mul(2.0, l.p1), x)), rn_mul(rn_mul(2.0, l.p2), y));
    j[2] = j[1];
    j[3] = rn_add(rn_add(rn_add(r.rad, rn_mul(rn_mul(2.0, r.yy), g)), rn_mul(rn_mul(6.0, l.p1), y)), rn_mul(rn_mul(2.0, l.p2), x));
    return rn_add(rn_mul(j[0], j[3]), -rn_mul(j[1], j[2]));
}

CWIPC_HOST_DEVICE CWIPC_FORCEINLINE double rgbd_abs(double a) { return a < 0.0 ? -a : a; }

// The ray table's entry for pixel (u, v) of a depth camera; false (and NaNs in out) when the pixel has no ray.
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_ray(const RgbdCamTerms &c, const RgbdLens &l, int u, int v, double out[2]) {
    const double xd = rn_div(rn_add((double)u, -c.cx), c.fx), yd = rn_div(rn_add((double)v, -c.cy), c.fy);
    out[0] = xd; out[1] = yd;
    if (rgbd_lens_is_pinhole(l)) return true;
    const double nan = __builtin_nan("");
    double x = xd, y = yd;
    for (int step = 0;; step++) {
        const RgbdRadial r = rgbd_radial(l, x, y);
        double at[2], j[4];
        rgbd_distort_with(l, r, x, y, at);
        const double ex = rn_add(at[0], -xd), ey = rn_add(at[1], -yd);
        const double det = rgbd_jacobian(l, r, x, y, j);
        if (rgbd_abs(ex) < RGBD_NEWTON_EPS && rgbd_abs(ey) < RGBD_NEWTON_EPS) {
            if (det > 0.0) { out[0] = x; out[1] = y; return true; }
            break;
        }
        if (step == RGBD_NEWTON_STEPS) break;
        x = rn_add(x, -rn_div(rn_add(rn_mul(j[3], ex), -rn_mul(j[1], ey)), det));
        y = rn_add(y, -rn_div(rn_add(rn_mul(j[0], ey), -rn_mul(j[2], ex)), det));
    }
    out[0] = nan; out[1] = nan;
    return false;
}

// The colour pixel of the point (xc, yc, z) in depth-camera coordinates and its Pz, the depth along the colour camera's axis; false:
// none (pz is then whatever the third row gave, a NaN included).
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_colour_pixel_depth(const RgbdColourTerms &c, double xc, double yc, double z, int out[2], double &pz) {
    double p[3];
    for (int row = 0; row < 3; row++) {
        const double *m = c.m + 4 * row;
        p[row] = rn_add(rn_add(rn_add(rn_mul(m[0], xc), rn_mul(m[1], yc)), rn_mul(m[2], z)), m[3]);
    }
    pz = p[2];
    if (!(p[2] > 0.0) || !(p[2] <= 1.7976931348623157e308)) return false;
    double at[2];
    rgbd_distort(c.lens, rn_div(p[0], p[2]), rn_div(p[1], p[2]), at);
    const double uc = __builtin_floor(rn_add(rn_add(rn_mul(c.fx, at[0]), c.cx), 0.5));
    const double vc = __builtin_floor(rn_add(rn_add(rn_mul(c.fy, at[1]), c.cy), 0.5));
    if (!(uc >= 0.0 && uc < (double)c.width && vc >= 0.0 && vc < (double)c.height)) return false;
    out[0] = (int)uc; out[1] = (int)vc;
    return true;
}

// The colour pixel of the point (xc, yc, z) in depth-camera coordinates; false: none.
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_colour_pixel(const RgbdColourTerms &c, double xc, double yc, double z, int out[2]) {
    double pz;
    return rgbd_colour_pixel_depth(c, xc, yc, z, out, pz);
}

constexpr int RGBD_MAX_SPLAT = 8;
constexpr unsigned long long RGBD_KEY_EMPTY = ~0ull;   // above the key of every finite Pz

// The z-buffer's word for a candidate's Pz (finite, > 0): its bits, which order as the doubles do.
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE unsigned long long rgbd_depth_key(double pz) {
    unsigned long long key;
    __builtin_memcpy(&key, &pz, sizeof key);
    return key;
}

// Is the candidate with depth pz occluded, key_min being the z-buffer's word at its own colour pixel?  (An empty word is a NaN: no.)
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_occluded(unsigned long long key_min, double pz, double margin) {
    double zmin;
    __builtin_memcpy(&zmin, &key_min, sizeof zmin);
    return zmin < rn_add(pz, -margin);
}

// The cells of a candidate's square that lie inside the colour image: columns lo[0] .. hi[0], rows lo[1] .. hi[1] (never empty: the
// candidate's own pixel is inside).  "q's square reaches p's pixel" and "q's pixel is in p's square" say the same, so Zmin at p's pixel
// is as well the minimum, over this box round p's pixel, of the per-cell minimum of the candidates that land ON a cell.
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void rgbd_splat_box(const RgbdColourTerms &c, const int at[2], int splat, int lo[2], int hi[2]) {
    lo[0] = at[0] - splat < 0 ? 0 : at[0] - splat;
    lo[1] = at[1] - splat < 0 ? 0 : at[1] - splat;
    hi[0] = at[0] + splat > c.width - 1 ? c.width - 1 : at[0] + splat;
    hi[1] = at[1] + splat > c.height - 1 ? c.height - 1 : at[1] + splat;
}

// xc, yc of a pixel with camera-axis depth z: from the ray (xn, yn), or rgbd_terms.hpp's for a sensor without depth coefficients
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void rgbd_raw_xy(const RgbdCamTerms &c, const double *ray, int u, int v, double z, double &xc, double &yc) {
    if (ray) {
        xc = rn_mul(ray[0], z); yc = rn_mul(ray[1], z);
    } else {
        xc = rgbd_xc(c, u, z); yc = rgbd_yc(c, v, z);
    }
}

// the point of pixel (u, v) with depth d: rgbd_point (rgbd_terms.hpp) with xc, yc from the ray where there is one
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE void rgbd_raw_point(const RgbdCamTerms &c, const double *ray, int u, int v, unsigned d, float out[3]) {
    const double z = rgbd_z(d, c.depth_scale);
    double xc, yc;
    rgbd_raw_xy(c, ray, u, v, z, xc, yc);
    for (int row = 0; row < 3; row++) out[row] = rgbd_world(c, row, xc, yc, z);
}

// rgbd_keep (rgbd_terms.hpp) for a pixel whose xc and yc come from a ray: the same four filters in the same order
template <class Colour>
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE bool rgbd_keep_ray(const RgbdCamTerms &c, const RgbdFilterTerms &f, unsigned active, const double *ray, unsigned d,
                                                       Colour colour) {
    if (d == 0u) return false;
    const double z = rgbd_z(d, c.depth_scale);
    if ((active & RGBD_DEPTH_RANGE) && (z < f.near_z || z > f.far_z)) return false;
    if (active & (RGBD_HEIGHT | RGBD_RADIUS)) {
        const double xc = rn_mul(ray[0], z), yc = rn_mul(ray[1], z);
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

// Erosion of one row's validity words.  own, left, right: 64 pixels each, bit i = pixel i has depth, bits outside the image SET (they
// do not erode).  Bit i of the result: pixels i - ex .. i + ex all have depth.  0 <= ex <= 32.
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE unsigned long long rgbd_erode_word(unsigned long long left, unsigned long long own, unsigned long long right, int ex) {
    unsigned long long acc = own;
    for (int s = 1; s <= ex; s++) {
        acc &= (own >> s) | (right << (64 - s));   // pixel i + s
        acc &= (own << s) | (left >> (64 - s));    // pixel i - s
    }
    return acc;
}

}  // namespace cwipc_amd
