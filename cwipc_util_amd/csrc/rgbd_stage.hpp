// rgbd_stage.hpp -- the RGB-D source's host staging, stated once: the plain structs its kernels are handed, what the entries refuse
// and in which order, a grab's options as one plan, and how every device block is carved -- each block has one function that gives
// its size and its parts.  Free of HIP: it compiles with a plain host C++ compiler, so the stand-alone host program of the tests
// (tests/abi/rgbd_stage_host.cpp) checks every carve for bounds and overlap and every refusal for its text without a GPU.
// internal.hpp includes it; rgbd.cpp (the aligned entry) and rgbd_rig.cpp (the raw entry) are its callers.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "cwipc_util_amd/hip_ext.h"
#include "rgbd_terms.hpp"
#include "rgbd_lens.hpp"
#include "rgbd_depthfilter.hpp"
#include "rgbd_decimate.hpp"
#include "codec_stage.hpp"   // (stage_round256)

namespace cwipc_amd {

namespace k {

// ---- kernels_rgbd.hip: cwipc_hip_from_rgbd (the contract is in rgbd_terms.hpp and hip_ext.h) ----
// One camera of a frame as the kernels see it; the cameras' pixels are numbered through, camera after camera, row-major: `first` is
// the number of this camera's pixel (0, 0).  depth and colour are device memory; colour is 4-byte aligned with at least 8 readable
// bytes behind its last pixel.
struct RgbdCamDev {
    RgbdCamTerms t;
    const uint16_t *depth;
    const uint8_t *colour;
    uint32_t width, bpp, tile, first;
};
// ---- the raw entry, cwipc_hip_rgbd_rig_grab (the contract is in rgbd_lens.hpp and hip_ext.h) ----
// One camera of a rig.  The RgbdCamDev part is the camera as count and scatter see it once the registration has run: depth is the
// (eroded, cleared) depth image, colour the REGISTERED image on the depth grid, bpp 3.  depth_rw and registered are those two again,
// to write through.  rays: the ray table (2 doubles per depth pixel), nullptr for a sensor without depth lens coefficients.
// raw_colour: the colour image as the camera sent it (raw_bpp bytes per pixel, ct.width x ct.height, 4-byte aligned, 8 readable
// bytes behind it).  The validity words of the erosion: wpr words per row, this camera's first is number wfirst.  The occlusion
// test's z-buffer: one word per colour pixel, row-major, this camera's first is number zfirst.  A decimated rig (rgbd_decimate.hpp): all
// of the above is on the decimated grid; full_depth is the depth image as the sensor delivers it, full_width pixels wide, 16-byte
// aligned with readable bytes up to the next 16-byte boundary behind it; nullptr without decimation.
struct RgbdRawCamDev : RgbdCamDev {
    uint16_t *depth_rw;
    uint8_t *registered;
    const double *rays;
    const uint8_t *raw_colour;
    RgbdColourTerms ct;
    uint32_t raw_bpp, height, wpr, wfirst;
    size_t zfirst;
    const uint16_t *full_depth;
    uint32_t full_width;
};

}  // namespace k

// ---- what a camera and a sensor are refused for ----
constexpr uint64_t RGBD_MAX_PIXELS = 0x7fffffffull;
constexpr const char *RGBD_TOO_MANY_PIXELS = "more than 2^31 - 1 pixels";

// The checks of one camera that do not look at its images; nullptr when it is fine, else what is wrong with it.
inline const char *rgbd_camera_problem(const cwipc_hip_rgbd_camera &cam) {
    if (cam.width < 1 || cam.height < 1) return "width and height must be at least 1";
    if (cam.bpp != 3 && cam.bpp != 4) return "bpp must be 3 (R, G, B) or 4 (B, G, R, A)";
    bool finite = std::isfinite(cam.fx) && std::isfinite(cam.fy) && std::isfinite(cam.cx) && std::isfinite(cam.cy) && std::isfinite(cam.depth_scale);
    for (int i = 0; i < 16; i++) finite = finite && std::isfinite(cam.trafo[i]);
    if (!finite) return "the intrinsics, depth_scale and the matrix must be finite";
    if (cam.fx == 0.0 || cam.fy == 0.0) return "fx and fy must not be zero";
    return nullptr;
}

inline const char *rgbd_sensor_problem(const cwipc_hip_rgbd_sensor &s) {
    if (s.width < 1 || s.height < 1 || s.colour_width < 1 || s.colour_height < 1) return "width and height must be at least 1";
    if ((uint64_t)s.colour_width * (uint64_t)s.colour_height > RGBD_MAX_PIXELS) return RGBD_TOO_MANY_PIXELS;
    if (s.colour_bpp != 3 && s.colour_bpp != 4) return "colour_bpp must be 3 (R, G, B) or 4 (B, G, R, A)";
    bool finite = std::isfinite(s.fx) && std::isfinite(s.fy) && std::isfinite(s.cx) && std::isfinite(s.cy) && std::isfinite(s.depth_scale) &&
                  std::isfinite(s.colour_fx) && std::isfinite(s.colour_fy) && std::isfinite(s.colour_cx) && std::isfinite(s.colour_cy);
    for (int i = 0; i < 8; i++) finite = finite && std::isfinite(s.coeffs[i]) && std::isfinite(s.colour_coeffs[i]);
    for (int i = 0; i < 16; i++) finite = finite && std::isfinite(s.trafo[i]) && std::isfinite(s.depth_to_colour[i]);
    if (!finite) return "the intrinsics, the lens coefficients, depth_scale and the matrices must be finite";
    if (s.fx == 0.0 || s.fy == 0.0 || s.colour_fx == 0.0 || s.colour_fy == 0.0) return "fx and fy must not be zero";
    return nullptr;
}

// Why cwipc_hip_from_rgbd refuses a frame before it looks for a device, the first reason in the order it has always tested them
// (camera after camera: its pointers, its numbers, the pixels so far); empty: it does not.
inline std::string rgbd_frame_refusal(const cwipc_hip_rgbd_camera *cams, int ncam, int attach_flags) {
    if (cams == nullptr) return "NULL argument";
    if (ncam <= 0) return "ncam must be at least 1";
    uint64_t total = 0;
    for (int k = 0; k < ncam; k++) {
        const cwipc_hip_rgbd_camera &cam = cams[k];
        if (cam.depth == nullptr || cam.colour == nullptr || (attach_flags != 0 && cam.serial == nullptr)) return "camera " + std::to_string(k) + ": NULL argument";
        if (const char *problem = rgbd_camera_problem(cam)) return "camera " + std::to_string(k) + ": " + problem;
        total += (uint64_t)cam.width * (uint64_t)cam.height;   // (each at most 2^62, checked before the next is added: no overflow)
        if (total > RGBD_MAX_PIXELS) return RGBD_TOO_MANY_PIXELS;
    }
    return std::string();
}

// The same for a rig of the caller's (full-size) sensors: the pixel limit counts the full-size depth images.
inline std::string rgbd_rig_refusal(const cwipc_hip_rgbd_sensor *sensors, int ncam, int decimation) {
    if (sensors == nullptr) return "NULL argument";
    if (ncam <= 0) return "ncam must be at least 1";
    if (decimation < 1 || decimation > RGBD_MAX_DECIMATION) return "decimation must be between 1 and 8";
    uint64_t full_total = 0;
    for (int k = 0; k < ncam; k++) {
        if (const char *problem = rgbd_sensor_problem(sensors[k])) return "camera " + std::to_string(k) + ": " + problem;
        if (sensors[k].width < decimation || sensors[k].height < decimation)
            return "camera " + std::to_string(k) + ": width and height must be at least the decimation";
        full_total += (uint64_t)sensors[k].width * (uint64_t)sensors[k].height;
        if (full_total > RGBD_MAX_PIXELS) return RGBD_TOO_MANY_PIXELS;
    }
    return std::string();
}

// ---- a grab's options ----
// What a grab does, from the four optional structs of the grab entries.  A stage that is off leaves its numbers 0, so that two sets
// of structs that ask for the same thing give the same plan, field for field.
struct RgbdGrabPlan {
    int ex = 0, ey = 0;                 // erosion (rule 1)
    int magnitude = 0;                  // rule 0a's iterations, 0: off
    RgbdSmoothTerms spatial{0, 0, 0};
    bool temporal = false;              // rule 0b
    RgbdSmoothTerms temporal_terms{0, 0, 0};
    int persistency = 0;
    int fill_mode = 0;                  // rule 0c, 0: off
    bool occluded = false;              // rules 3a and 3b in place of the plain registration
    int splat = 0;
    double margin = 0.0;
};

// what is wrong with a smoothing stage's numbers, to follow "spatial_" or "temporal_"; nullptr: nothing
inline const char *rgbd_smooth_problem(double alpha, double delta) {
    if (!(std::isfinite(alpha) && alpha > 0.0 && alpha <= 1.0)) return "alpha must be greater than 0 and at most 1";
    if (!(std::isfinite(delta) && delta > 0.0)) return "delta must be finite and greater than 0";
    return nullptr;
}

// The plan of (holefill, depthfilter, prep, occlusion), each of which may be NULL: off.  Returns the first problem in the order the
// entries have always named them -- erosion, splat, margin, magnitude, persistency (judged whether the temporal stage is on or not),
// the spatial numbers and the temporal numbers (each only when its stage is on), the fill mode -- or nothing, and then `plan` is set.
inline std::string rgbd_grab_plan(const cwipc_hip_rgbd_holefill *holefill, const cwipc_hip_rgbd_depthfilter *depthfilter, const cwipc_hip_rgbd_prep *prep,
                                  const cwipc_hip_rgbd_occlusion *occlusion, RgbdGrabPlan &plan) {
    RgbdGrabPlan p;
    if (prep) { p.ex = prep->depth_x_erosion; p.ey = prep->depth_y_erosion; }
    if (p.ex < 0 || p.ex > RGBD_MAX_EROSION || p.ey < 0 || p.ey > RGBD_MAX_EROSION) return "depth_x_erosion and depth_y_erosion must be between 0 and 32";
    if (occlusion) {
        if (occlusion->splat < 0 || occlusion->splat > RGBD_MAX_SPLAT) return "occlusion: splat must be between 0 and 8";
        if (!(std::isfinite(occlusion->margin) && occlusion->margin >= 0.0)) return "occlusion: margin must be finite and not negative";
        p.occluded = true; p.splat = occlusion->splat; p.margin = occlusion->margin;
    }
    if (depthfilter) {
        const cwipc_hip_rgbd_depthfilter &d = *depthfilter;
        if (d.spatial_magnitude < 0 || d.spatial_magnitude > RGBD_MAX_SPATIAL_MAGNITUDE) return "depthfilter: spatial_magnitude must be between 0 and 5";
        if (d.temporal_persistency < 0 || d.temporal_persistency > RGBD_MAX_PERSISTENCY) return "depthfilter: temporal_persistency must be between 0 and 8";
        if (d.spatial_magnitude > 0) {
            if (const char *problem = rgbd_smooth_problem(d.spatial_alpha, d.spatial_delta)) return std::string("depthfilter: spatial_") + problem;
            p.magnitude = d.spatial_magnitude; p.spatial = rgbd_smooth_terms(d.spatial_alpha, d.spatial_delta);
        }
        if (d.temporal != 0) {
            if (const char *problem = rgbd_smooth_problem(d.temporal_alpha, d.temporal_delta)) return std::string("depthfilter: temporal_") + problem;
            p.temporal = true; p.temporal_terms = rgbd_smooth_terms(d.temporal_alpha, d.temporal_delta); p.persistency = d.temporal_persistency;
        }
    }
    if (holefill) p.fill_mode = holefill->mode;
    if (p.fill_mode < 0 || p.fill_mode > RGBD_MAX_HOLEFILL) return "holefill: mode must be between 0 and 3";
    plan = p;
    return std::string();
}

// ---- the images a call is handed ----
struct RgbdFrameBytes { size_t depth, colour; };
inline RgbdFrameBytes rgbd_frame_bytes(const cwipc_hip_rgbd_camera &cam) {
    const size_t npix = (size_t)cam.width * (size_t)cam.height;
    return {npix * 2, npix * (size_t)cam.bpp};
}
// (of a rig's camera: the caller's full-size sensor, not the one on the rig's grid)
inline RgbdFrameBytes rgbd_frame_bytes(const cwipc_hip_rgbd_sensor &full) {
    return {(size_t)full.width * (size_t)full.height * 2, (size_t)full.colour_width * (size_t)full.colour_height * (size_t)full.colour_bpp};
}

// ---- device blocks ----
// Every part starts on a 256-byte boundary and is rounded up to one.  Behind a colour or registered image 8 more bytes are readable:
// the kernels read a 3-byte pixel as a pair of dwords.  Offsets are from the block's start; the table of cameras is its first part.

// The aligned frame's block (cwipc_hip_from_rgbd): the table | per camera its depth image, its colour image.
struct RgbdFrameLayout {
    struct Cam { size_t depth, colour; uint32_t first; };
    size_t table_bytes = 0, bytes = 0;
    uint32_t total = 0;   // pixels
    std::vector<Cam> cams;
};
inline RgbdFrameLayout rgbd_frame_layout(const cwipc_hip_rgbd_camera *cams, int ncam) {
    RgbdFrameLayout l;
    l.bytes = l.table_bytes = stage_round256((size_t)ncam * sizeof(k::RgbdCamDev));
    for (int k = 0; k < ncam; k++) {
        const RgbdFrameBytes b = rgbd_frame_bytes(cams[k]);
        RgbdFrameLayout::Cam c;
        c.first = l.total;
        c.depth = l.bytes;
        c.colour = c.depth + stage_round256(b.depth);
        l.bytes = c.colour + stage_round256(b.colour + 8);
        l.total += (uint32_t)(b.depth / 2);
        l.cams.push_back(c);
    }
    return l;
}

// A sensor on a rig's grid (RULE D); decimation 1: the sensor itself (it would give the same bits: a subtraction of 0, divisions by 1).
inline cwipc_hip_rgbd_sensor rgbd_grid_sensor(cwipc_hip_rgbd_sensor s, int decimation) {
    if (decimation > 1) {
        const RgbdGrid g = rgbd_derived_grid(s.width, s.height, s.fx, s.fy, s.cx, s.cy, decimation);
        s.width = g.width; s.height = g.height; s.fx = g.fx; s.fy = g.fy; s.cx = g.cx; s.cy = g.cy;
    }
    return s;
}

inline RgbdLens rgbd_lens_of(const double k[8]) {
    RgbdLens l;
    l.k1 = k[0]; l.k2 = k[1]; l.p1 = k[2]; l.p2 = k[3]; l.k3 = k[4]; l.k4 = k[5]; l.k5 = k[6]; l.k6 = k[7];
    return l;
}

// The rig's block: the table | per camera its ray table (none, offset 0, for a pinhole depth lens), depth plane, raw colour image,
// registered image and -- a decimated rig only, else offset 0 -- the full-size depth plane (256-byte aligned and rounded: the
// decimation kernel's 16-byte loads stay inside it) | the erosion's validity words.  grid: the sensors on the rig's grid; full: the caller's.
struct RgbdRigLayout {
    struct Cam {
        size_t rays, depth, raw_colour, registered, full_depth;
        uint32_t first, wpr, wfirst;   // the first pixel; validity words per row and the first of them
        size_t zfirst;                 // the first z-buffer word
    };
    size_t table_bytes = 0, words = 0, bytes = 0;
    size_t zwords = 0;                     // one per colour pixel of every camera: the z-buffer is a block of its own
    uint32_t total = 0, total_words = 0;   // depth pixels on the grid; validity words
    std::vector<Cam> cams;
};
inline RgbdRigLayout rgbd_rig_layout(const cwipc_hip_rgbd_sensor *grid, const cwipc_hip_rgbd_sensor *full, int ncam, int decimation) {
    RgbdRigLayout l;
    size_t at = l.table_bytes = stage_round256((size_t)ncam * sizeof(k::RgbdRawCamDev));
    const auto part = [&at](size_t bytes) { const size_t here = at; at += stage_round256(bytes); return here; };
    for (int k = 0; k < ncam; k++) {
        const cwipc_hip_rgbd_sensor &s = grid[k];
        const size_t npix = (size_t)s.width * (size_t)s.height, ncol = (size_t)s.colour_width * (size_t)s.colour_height;
        RgbdRigLayout::Cam c;
        c.rays = rgbd_lens_is_pinhole(rgbd_lens_of(s.coeffs)) ? 0 : part(npix * 16);
        c.depth = part(npix * 2);
        c.raw_colour = part(ncol * (size_t)s.colour_bpp + 8);
        c.registered = part(npix * 3 + 8);
        c.full_depth = decimation > 1 ? part(rgbd_frame_bytes(full[k]).depth) : 0;
        c.first = l.total; c.wpr = (uint32_t)(((uint64_t)s.width + 63) / 64); c.wfirst = l.total_words; c.zfirst = l.zwords;
        l.total += (uint32_t)npix;
        l.total_words += (uint32_t)s.height * c.wpr;
        l.zwords += ncol;
        l.cams.push_back(c);
    }
    l.words = part((size_t)l.total_words * 8);
    l.bytes = at;
    return l;
}

// The temporal filter's state, a block of its own: `total` doubles (the running values) | `total` bytes (the histories), both in
// pixel-number order; a camera's part of either starts at its `first`.
struct RgbdStateLayout {
    size_t history, bytes;
    size_t value_at(uint32_t first) const { return (size_t)first * sizeof(double); }
    size_t history_at(uint32_t first) const { return history + first; }
};
inline RgbdStateLayout rgbd_state_layout(uint32_t total) {
    const size_t history = stage_round256((size_t)total * sizeof(double));
    return {history, history + (size_t)total};
}

}  // namespace cwipc_amd
