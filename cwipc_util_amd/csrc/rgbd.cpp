// rgbd.cpp -- the RGB-D source end: cwipc_hip_from_rgbd builds one device-resident cloud from the cameras' depth and colour images,
// the step a capturer plug-in of the reference does on the host (its shared per-point filters: reference
// include/cwipc_util/internal/capturers.hpp:208-275).  Host orchestration only: the arithmetic is rgbd_terms.hpp's, the kernels are
// kernels_rgbd.hip's.  The images go up with asynchronous copies on the calling thread's stream (from where they lie when the caller
// holds them in page-locked memory, through the thread's pinned staging buffer otherwise) together with one small table of cameras;
// the point count comes back in a pinned word.  The two mappings a grabber answers for the registration tooling are here too, on the
// host.  There is NO CPU fallback for the cloud: without a usable GPU the call logs an ERROR and returns NULL.
//
// The raw entry (cwipc_hip_rgbd_rig_*, rgbd_lens.hpp) keeps what is constant per camera in a rig: the camera table, the ray tables
// (computed here at creation) and the frame's device buffers, so that a grab uploads the images and nothing else.  The occlusion test
// (cwipc_hip_rgbd_rig_grab_occluded) adds a z-buffer of the colour grids, which the first grab that asks for it allocates.  The depth
// post-processing (cwipc_hip_rgbd_rig_grab_filtered, rgbd_depthfilter.hpp) adds the temporal filter's per-pixel state in the same way.
// A decimated rig (cwipc_hip_rgbd_rig_create_decimated, rgbd_decimate.hpp) keeps the caller's sensors for the size of the uploads and
// derived ones for everything else; hole filling (cwipc_hip_rgbd_rig_grab_filled) adds a scratch depth plane as the z-buffer is added.
#include "internal.hpp"

#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace cwipc_amd;

namespace {

// The checks of one camera that do not look at its images; nullptr when it is fine, else what is wrong with it.
const char *camera_problem(const cwipc_hip_rgbd_camera &cam) {
    if (cam.width < 1 || cam.height < 1) return "width and height must be at least 1";
    if (cam.bpp != 3 && cam.bpp != 4) return "bpp must be 3 (R, G, B) or 4 (B, G, R, A)";
    bool finite = std::isfinite(cam.fx) && std::isfinite(cam.fy) && std::isfinite(cam.cx) && std::isfinite(cam.cy) && std::isfinite(cam.depth_scale);
    for (int i = 0; i < 16; i++) finite = finite && std::isfinite(cam.trafo[i]);
    if (!finite) return "the intrinsics, depth_scale and the matrix must be finite";
    if (cam.fx == 0.0 || cam.fy == 0.0) return "fx and fy must not be zero";
    return nullptr;
}

RgbdCamTerms camera_terms(const cwipc_hip_rgbd_camera &cam) {
    RgbdCamTerms t;
    t.fx = cam.fx; t.fy = cam.fy; t.cx = cam.cx; t.cy = cam.cy; t.depth_scale = cam.depth_scale;
    for (int i = 0; i < 12; i++) t.m[i] = cam.trafo[i];
    return t;
}

size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// `bytes` of an image on their way to dev: straight from the caller's page-locked memory, or through the staging buffer at *stage
// (which moves on)
bool upload(const void *src, size_t bytes, uint8_t *dev, uint8_t **stage, hipStream_t stream) {
    const void *from = src;
    if (!host_range_device_alias(src, bytes)) {
        parallel_memcpy(*stage, src, bytes);
        from = *stage;
        *stage += round256(bytes);
    }
    return hipMemcpyAsync(dev, from, bytes, hipMemcpyHostToDevice, stream) == hipSuccess;
}

void attach_image(cwipc_metadata *meta, const std::string &name, const cwipc_hip_rgbd_camera &cam, int bpp, const void *data) {
    const size_t bytes = (size_t)cam.width * (size_t)cam.height * (size_t)bpp;
    void *copy = malloc(bytes);
    if (!copy) return;
    memcpy(copy, data, bytes);
    meta->_add(name, "width=" + std::to_string(cam.width) + ",height=" + std::to_string(cam.height) + ",bpp=" + std::to_string(bpp), copy, bytes, ::free);
}

// The caller's errorMessage is where the log's errors go for as long as an entry point runs.
struct ErrorbufScope {
    explicit ErrorbufScope(char **errorMessage) { cwipc_log_set_errorbuf(errorMessage); }
    ~ErrorbufScope() { cwipc_log_set_errorbuf(nullptr); }
};

RgbdFilterTerms filter_terms(const cwipc_hip_rgbd_filter *filter) {
    RgbdFilterTerms f{};
    if (filter) {
        f.near_z = filter->threshold_near; f.far_z = filter->threshold_far;
        f.height_min = filter->height_min; f.height_max = filter->height_max;
        f.radius = filter->radius; f.green = filter->greenscreen;
    }
    return f;
}

// After the stream has been waited for (ok: everything until then went well): the cloud of the `kept` points the scan published under
// `tag`, in dst's planes (room for total points) or, when few survive, in planes of their own.  nullptr: the error has been noted.
cwipc_hip_pointcloud *finish_cloud(const char *who, ThreadCtx &c, bool ok, uint32_t tag, std::shared_ptr<DeviceSoA> dst, const uint32_t tiles[8],
                                   uint64_t timestamp, float cellsize) {
    const PinnedReport report = c.report();
    const size_t kept = report.value(0);
    if (!ok || !report.landed(tag, 0) || kept > dst->npoints) {
        if (ok) note_error(who, "inconsistent point count");
        else if (!*cwipc_hip_last_error()) note_error(who, "a kernel or a copy failed");
        else cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, cwipc_hip_last_error());
        return nullptr;
    }
    dst = soa_keep(dst, kept, who);   // (as a compaction's result)
    if (!dst) return nullptr;
    dst->set_tiles(tiles);
    auto *rv = new cwipc_hip_pointcloud();
    rv->adopt_device(dst, timestamp, cellsize);
    return rv;
}

}  // namespace

extern "C" cwipc_pointcloud *cwipc_hip_from_rgbd(const cwipc_hip_rgbd_camera *cams, int ncam, const cwipc_hip_rgbd_filter *filter, uint64_t timestamp,
                                                 float cellsize, int attach_flags, char **errorMessage) {
    const char *who = "cwipc_hip_from_rgbd";
    ErrorbufScope errors(errorMessage);
    if (cams == nullptr || ncam <= 0) {
        note_error(who, cams == nullptr ? "NULL argument" : "ncam must be at least 1");
        return nullptr;
    }
    uint64_t total = 0;
    size_t image_bytes = 0, staged_bytes = 0;
    for (int k = 0; k < ncam; k++) {
        const cwipc_hip_rgbd_camera &cam = cams[k];
        if (cam.depth == nullptr || cam.colour == nullptr || (attach_flags != 0 && cam.serial == nullptr)) {
            note_error(who, "camera " + std::to_string(k) + ": NULL argument");
            return nullptr;
        }
        if (const char *problem = camera_problem(cam)) {
            note_error(who, "camera " + std::to_string(k) + ": " + problem);
            return nullptr;
        }
        const size_t npix = (size_t)cam.width * (size_t)cam.height;
        total += npix;
        if (total > 0x7fffffffull) {
            note_error(who, "more than 2^31 - 1 pixels");
            return nullptr;
        }
        image_bytes += round256(npix * 2) + round256(npix * (size_t)cam.bpp + 8);   // (8: the kernel reads a 3-byte pixel as a pair of dwords)
        if (!host_range_device_alias(cam.depth, npix * 2)) staged_bytes += round256(npix * 2);
        if (!host_range_device_alias(cam.colour, npix * (size_t)cam.bpp)) staged_bytes += round256(npix * (size_t)cam.bpp);
    }
    if (!device_available(who)) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;

    const RgbdFilterTerms f = filter_terms(filter);
    // one device block: the table of cameras | every camera's depth image | its colour image, each part on a 256-byte boundary
    const size_t table_bytes = round256((size_t)ncam * sizeof(k::RgbdCamDev));
    const size_t nb = k::rgbd_blocks((uint32_t)total);
    uint8_t *dev = (uint8_t *)pool_alloc(table_bytes + image_bytes);
    uint8_t *host = (uint8_t *)c.staging(table_bytes + staged_bytes);
    uint32_t *counts = (uint32_t *)c.device_scratch((nb + 1) * sizeof(uint32_t));
    auto dst = soa_alloc((size_t)total);
    if (!dev || !host || !counts || !dst) {
        pool_free(dev);
        note_error(who, "out of memory");
        return nullptr;
    }
    k::RgbdCamDev *table = (k::RgbdCamDev *)host;
    uint8_t *stage = host + table_bytes, *at = dev + table_bytes;
    uint32_t first = 0, tiles[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = true;
    for (int k = 0; k < ncam && ok; k++) {
        const cwipc_hip_rgbd_camera &cam = cams[k];
        const size_t npix = (size_t)cam.width * (size_t)cam.height;
        k::RgbdCamDev &t = table[k];
        t.t = camera_terms(cam);
        t.depth = (const uint16_t *)at;
        ok = upload(cam.depth, npix * 2, at, &stage, c.stream);
        at += round256(npix * 2);
        t.colour = at;
        ok = ok && upload(cam.colour, npix * (size_t)cam.bpp, at, &stage, c.stream);
        at += round256(npix * (size_t)cam.bpp + 8);
        t.width = (uint32_t)cam.width; t.bpp = (uint32_t)cam.bpp; t.tile = cam.tile; t.first = first;
        first += (uint32_t)npix;
        tiles[cam.tile >> 5] |= 1u << (cam.tile & 31u);
    }
    ok = ok && hipMemcpyAsync(dev, table, (size_t)ncam * sizeof(k::RgbdCamDev), hipMemcpyHostToDevice, c.stream) == hipSuccess;
    // the scan publishes the point count with this tag in the upper half of the first 64-bit pinned word (as the compaction driver's)
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 1);
    if (ok) {
        k::rgbd_count((const k::RgbdCamDev *)dev, ncam, (uint32_t)total, f, counts, c.tickets, report.device(), tag, c.stream);
        k::rgbd_scatter((const k::RgbdCamDev *)dev, ncam, (uint32_t)total, f, counts, *dst, c.stream);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;   // (also on failure: copies that read the staging buffer and kernels that write the planes may be in flight)
    pool_free(dev);
    cwipc_hip_pointcloud *rv = finish_cloud(who, c, ok, tag, dst, tiles, timestamp, cellsize);
    if (!rv) return nullptr;
    if (attach_flags & (CWIPC_HIP_RGBD_ATTACH_RGB | CWIPC_HIP_RGBD_ATTACH_DEPTH)) {
        cwipc_metadata *meta = rv->access_metadata();
        for (int k = 0; k < ncam; k++) {
            if (attach_flags & CWIPC_HIP_RGBD_ATTACH_RGB) attach_image(meta, std::string("rgb.") + cams[k].serial, cams[k], cams[k].bpp, cams[k].colour);
            if (attach_flags & CWIPC_HIP_RGBD_ATTACH_DEPTH) attach_image(meta, std::string("depth.") + cams[k].serial, cams[k], 2, cams[k].depth);
        }
    }
    return rv;
}

extern "C" int cwipc_hip_rgbd_map2d3d(const cwipc_hip_rgbd_camera *cam, int u, int v, int d, float out[3]) {
    if (cam == nullptr || out == nullptr || d <= 0 || camera_problem(*cam) != nullptr) return 0;
    rgbd_point(camera_terms(*cam), u, v, (unsigned)d, out);
    return 1;
}

extern "C" int cwipc_hip_rgbd_mapcolordepth(const cwipc_hip_rgbd_camera *cam, int u, int v, int out[2]) {
    if (cam == nullptr || out == nullptr || u < 0 || v < 0 || u >= cam->width || v >= cam->height) return 0;
    out[0] = u;
    out[1] = v;
    return 1;
}

// ---------------------------------------------------------------------------
// the raw entry: a rig of sensors (hip_ext.h: cwipc_hip_rgbd_rig_*)
// ---------------------------------------------------------------------------

struct cwipc_hip_rgbd_rig {
    int device = -1;
    std::vector<cwipc_hip_rgbd_sensor> sensors;  // on the rig's grid: the caller's when decimation == 1, else derived from them (RULE D)
    std::vector<cwipc_hip_rgbd_sensor> full;     // the caller's: the size of the depth images a grab is handed
    int decimation = 1;
    std::vector<std::string> serials;            // copies; has_serial says which sensors had one
    std::vector<bool> has_serial;
    std::vector<std::vector<double>> rays;       // per camera 2 * W * H doubles
    std::vector<k::RgbdRawCamDev> table;         // the host copy of the device table
    uint8_t *dev = nullptr;                      // one pool block: the table | per camera its ray table, depth, colour and registered image | the words
    unsigned long long *words = nullptr;
    unsigned long long *zbuf = nullptr;          // the occlusion test's z-buffer: a pool block of its own, made by the first occluded grab
    size_t zwords = 0;                           // one word per colour pixel of every camera
    uint8_t *state = nullptr;                    // the temporal filter's state: a pool block of its own, made by the first temporal grab:
                                                 // total doubles (the running values) | total bytes (the histories), in pixel-number order
    bool state_empty = true;                     // the state is to be read as all zero: the next temporal grab clears it first
    uint16_t *fill = nullptr;                    // hole filling from around: a depth plane of `total` pixels, a pool block of its own, made by the
                                                 // first grab that needs it
    uint32_t rows = 0, decimate_tiles = 0;       // every camera's rows; the decimation kernel's workgroups
    uint32_t row_groups = 0, col_groups = 0;     // the spatial filter's workgroups: every camera's rows and columns in groups
    uint32_t total = 0, total_words = 0;
    uint32_t tiles[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::mutex lock;                             // one grab at a time: the frame's device buffers are the rig's
};

namespace {

RgbdLens lens_of(const double k[8]) {
    RgbdLens l;
    l.k1 = k[0]; l.k2 = k[1]; l.p1 = k[2]; l.p2 = k[3]; l.k3 = k[4]; l.k4 = k[5]; l.k5 = k[6]; l.k6 = k[7];
    return l;
}

const char *sensor_problem(const cwipc_hip_rgbd_sensor &s) {
    if (s.width < 1 || s.height < 1 || s.colour_width < 1 || s.colour_height < 1) return "width and height must be at least 1";
    if ((uint64_t)s.colour_width * (uint64_t)s.colour_height > 0x7fffffffull) return "more than 2^31 - 1 pixels";
    if (s.colour_bpp != 3 && s.colour_bpp != 4) return "colour_bpp must be 3 (R, G, B) or 4 (B, G, R, A)";
    bool finite = std::isfinite(s.fx) && std::isfinite(s.fy) && std::isfinite(s.cx) && std::isfinite(s.cy) && std::isfinite(s.depth_scale) &&
                  std::isfinite(s.colour_fx) && std::isfinite(s.colour_fy) && std::isfinite(s.colour_cx) && std::isfinite(s.colour_cy);
    for (int i = 0; i < 8; i++) finite = finite && std::isfinite(s.coeffs[i]) && std::isfinite(s.colour_coeffs[i]);
    for (int i = 0; i < 16; i++) finite = finite && std::isfinite(s.trafo[i]) && std::isfinite(s.depth_to_colour[i]);
    if (!finite) return "the intrinsics, the lens coefficients, depth_scale and the matrices must be finite";
    if (s.fx == 0.0 || s.fy == 0.0 || s.colour_fx == 0.0 || s.colour_fy == 0.0) return "fx and fy must not be zero";
    return nullptr;
}

RgbdCamTerms sensor_terms(const cwipc_hip_rgbd_sensor &s) {
    RgbdCamTerms t;
    t.fx = s.fx; t.fy = s.fy; t.cx = s.cx; t.cy = s.cy; t.depth_scale = s.depth_scale;
    for (int i = 0; i < 12; i++) t.m[i] = s.trafo[i];
    return t;
}

RgbdColourTerms colour_terms(const cwipc_hip_rgbd_sensor &s) {
    RgbdColourTerms t;
    t.fx = s.colour_fx; t.fy = s.colour_fy; t.cx = s.colour_cx; t.cy = s.colour_cy;
    t.lens = lens_of(s.colour_coeffs);
    for (int i = 0; i < 12; i++) t.m[i] = s.depth_to_colour[i];
    t.width = s.colour_width; t.height = s.colour_height;
    return t;
}

// what is wrong with a smoothing stage's numbers, to follow "spatial_" or "temporal_"; nullptr: nothing
const char *smooth_problem(double alpha, double delta) {
    if (!(std::isfinite(alpha) && alpha > 0.0 && alpha <= 1.0)) return "alpha must be greater than 0 and at most 1";
    if (!(std::isfinite(delta) && delta > 0.0)) return "delta must be finite and greater than 0";
    return nullptr;
}

bool rig_camera_ok(const cwipc_hip_rgbd_rig *rig, int cam) { return rig != nullptr && cam >= 0 && (size_t)cam < rig->sensors.size(); }

// cwipc_hip_rgbd_rig_create (decimation 1) and cwipc_hip_rgbd_rig_create_decimated
cwipc_hip_rgbd_rig *rig_create(const char *who, const cwipc_hip_rgbd_sensor *sensors, int ncam, int decimation, char **errorMessage) {
    ErrorbufScope errors(errorMessage);
    if (sensors == nullptr || ncam <= 0) {
        note_error(who, sensors == nullptr ? "NULL argument" : "ncam must be at least 1");
        return nullptr;
    }
    if (decimation < 1 || decimation > RGBD_MAX_DECIMATION) {
        note_error(who, "decimation must be between 1 and 8");
        return nullptr;
    }
    uint64_t total = 0, total_words = 0, full_total = 0;
    for (int k = 0; k < ncam; k++) {
        if (const char *problem = sensor_problem(sensors[k])) {
            note_error(who, "camera " + std::to_string(k) + ": " + problem);
            return nullptr;
        }
        if (sensors[k].width < decimation || sensors[k].height < decimation) {
            note_error(who, "camera " + std::to_string(k) + ": width and height must be at least the decimation");
            return nullptr;
        }
        const uint64_t width = (uint64_t)(sensors[k].width / decimation), height = (uint64_t)(sensors[k].height / decimation);
        total += width * height;
        total_words += height * ((width + 63) / 64);
        full_total += (uint64_t)sensors[k].width * (uint64_t)sensors[k].height;
        if (full_total > 0x7fffffffull) {
            note_error(who, "more than 2^31 - 1 pixels");
            return nullptr;
        }
    }
    if (!device_available(who)) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;

    std::unique_ptr<cwipc_hip_rgbd_rig> rig(new cwipc_hip_rgbd_rig());
    rig->device = current_device();
    rig->sensors.assign(sensors, sensors + ncam);
    rig->full.assign(sensors, sensors + ncam);
    rig->decimation = decimation;
    rig->total = (uint32_t)total;
    rig->total_words = (uint32_t)total_words;
    rig->table.resize((size_t)ncam);
    rig->rays.resize((size_t)ncam);
    const size_t table_bytes = round256((size_t)ncam * sizeof(k::RgbdRawCamDev));
    size_t bytes = table_bytes;
    for (int k = 0; k < ncam; k++) {
        cwipc_hip_rgbd_sensor &s = rig->sensors[(size_t)k];
        rig->has_serial.push_back(s.serial != nullptr);
        rig->serials.push_back(s.serial ? s.serial : "");
        s.serial = nullptr;   // (the caller's string is not kept)
        rig->full[(size_t)k].serial = nullptr;
        if (decimation > 1) {   // (1 would give the same bits: a subtraction of 0, divisions by 1)
            const RgbdGrid g = rgbd_derived_grid(s.width, s.height, s.fx, s.fy, s.cx, s.cy, decimation);
            s.width = g.width; s.height = g.height; s.fx = g.fx; s.fy = g.fy; s.cx = g.cx; s.cy = g.cy;
        }
        const size_t npix = (size_t)s.width * (size_t)s.height, ncol = (size_t)s.colour_width * (size_t)s.colour_height;
        const RgbdCamTerms t = sensor_terms(s);
        const RgbdLens lens = lens_of(s.coeffs);
        std::vector<double> &rays = rig->rays[(size_t)k];
        rays.resize(2 * npix);
        for (int v = 0; v < s.height; v++)
            for (int u = 0; u < s.width; u++) rgbd_ray(t, lens, u, v, &rays[2 * ((size_t)v * (size_t)s.width + (size_t)u)]);
        if (!rgbd_lens_is_pinhole(lens)) bytes += round256(npix * 16);
        bytes += round256(npix * 2) + round256(ncol * (size_t)s.colour_bpp + 8) + round256(npix * 3 + 8);
        if (decimation > 1) bytes += round256((size_t)rig->full[(size_t)k].width * (size_t)rig->full[(size_t)k].height * 2);
        rig->tiles[s.tile >> 5] |= 1u << (s.tile & 31u);
    }
    bytes += round256((size_t)total_words * 8);
    rig->dev = (uint8_t *)pool_alloc(bytes);
    if (!rig->dev) {
        note_error(who, "out of memory");
        return nullptr;
    }
    uint8_t *at = rig->dev + table_bytes;
    uint32_t first = 0, wfirst = 0;
    bool ok = true;
    for (int k = 0; k < ncam; k++) {
        const cwipc_hip_rgbd_sensor &s = rig->sensors[(size_t)k];
        const size_t npix = (size_t)s.width * (size_t)s.height, ncol = (size_t)s.colour_width * (size_t)s.colour_height;
        k::RgbdRawCamDev &t = rig->table[(size_t)k];
        t.zfirst = rig->zwords;
        rig->zwords += ncol;
        t.t = sensor_terms(s);
        t.ct = colour_terms(s);
        t.rays = nullptr;
        if (!rgbd_lens_is_pinhole(lens_of(s.coeffs))) {
            t.rays = (const double *)at;
            ok = ok && hipMemcpyAsync(at, rig->rays[(size_t)k].data(), npix * 16, hipMemcpyHostToDevice, c.stream) == hipSuccess;
            at += round256(npix * 16);
        }
        t.depth_rw = (uint16_t *)at; t.depth = t.depth_rw;
        at += round256(npix * 2);
        t.raw_colour = at;
        at += round256(ncol * (size_t)s.colour_bpp + 8);
        t.registered = at; t.colour = t.registered;
        at += round256(npix * 3 + 8);
        t.full_depth = nullptr; t.full_width = 0;
        if (decimation > 1) {   // (256-byte aligned and rounded: the decimation kernel's 16-byte loads stay inside it)
            const cwipc_hip_rgbd_sensor &whole = rig->full[(size_t)k];
            t.full_depth = (const uint16_t *)at; t.full_width = (uint32_t)whole.width;
            at += round256((size_t)whole.width * (size_t)whole.height * 2);
        }
        t.width = (uint32_t)s.width; t.height = (uint32_t)s.height; t.bpp = 3u; t.raw_bpp = (uint32_t)s.colour_bpp; t.tile = s.tile;
        t.first = first; t.wpr = (uint32_t)(((uint64_t)s.width + 63) / 64); t.wfirst = wfirst;
        first += (uint32_t)npix;
        wfirst += t.height * t.wpr;
        rig->row_groups += k::rgbd_line_groups(t.height);
        rig->col_groups += k::rgbd_line_groups(t.width);
        rig->rows += t.height;
        rig->decimate_tiles += k::rgbd_decimate_tiles(t.width, t.height);
    }
    rig->words = (unsigned long long *)at;
    ok = ok && hipMemcpyAsync(rig->dev, rig->table.data(), (size_t)ncam * sizeof(k::RgbdRawCamDev), hipMemcpyHostToDevice, c.stream) == hipSuccess;
    ok = c.sync() && ok;   // (the copies read the rig's vectors: they stay, but the next call may come from another thread)
    if (!ok) {
        if (!*cwipc_hip_last_error()) note_error(who, "a copy failed");
        else cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, cwipc_hip_last_error());
        pool_free(rig->dev);
        return nullptr;
    }
    return rig.release();
}

}  // namespace

extern "C" cwipc_hip_rgbd_rig *cwipc_hip_rgbd_rig_create(const cwipc_hip_rgbd_sensor *sensors, int ncam, char **errorMessage) {
    return rig_create("cwipc_hip_rgbd_rig_create", sensors, ncam, 1, errorMessage);
}

extern "C" cwipc_hip_rgbd_rig *cwipc_hip_rgbd_rig_create_decimated(const cwipc_hip_rgbd_sensor *sensors, int ncam, int decimation, char **errorMessage) {
    return rig_create("cwipc_hip_rgbd_rig_create_decimated", sensors, ncam, decimation, errorMessage);
}

extern "C" int cwipc_hip_rgbd_rig_decimation(const cwipc_hip_rgbd_rig *rig) { return rig ? rig->decimation : 0; }

extern "C" void cwipc_hip_rgbd_rig_free(cwipc_hip_rgbd_rig *rig) {
    if (rig == nullptr) return;
    pool_free(rig->dev);
    pool_free(rig->zbuf);
    pool_free(rig->state);
    pool_free(rig->fill);
    delete rig;
}

namespace {

// cwipc_hip_rgbd_rig_grab (occlusion == nullptr) and cwipc_hip_rgbd_rig_grab_occluded: one flow, the occlusion test's two steps in
// place of the plain registration when it is asked for; and cwipc_hip_rgbd_rig_grab_filtered, which puts the depth post-processing
// (rgbd_depthfilter.hpp) in front of it all when depthfilter has a stage that is on; and cwipc_hip_rgbd_rig_grab_filled, which fills
// holes (rgbd_decimate.hpp) between that and the erosion.  A decimated rig decimates the depth images before any of it.
cwipc_pointcloud *rig_grab(const char *who, cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_holefill *holefill,
                           const cwipc_hip_rgbd_depthfilter *depthfilter, const cwipc_hip_rgbd_prep *prep, const cwipc_hip_rgbd_occlusion *occlusion,
                           const cwipc_hip_rgbd_filter *filter,
                           uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage) {
    ErrorbufScope errors(errorMessage);
    if (rig == nullptr || frames == nullptr) {
        note_error(who, "NULL argument");
        return nullptr;
    }
    const int ncam = (int)rig->sensors.size();
    const int ex = prep ? prep->depth_x_erosion : 0, ey = prep ? prep->depth_y_erosion : 0;
    if (ex < 0 || ex > RGBD_MAX_EROSION || ey < 0 || ey > RGBD_MAX_EROSION) {
        note_error(who, "depth_x_erosion and depth_y_erosion must be between 0 and 32");
        return nullptr;
    }
    if (occlusion && (occlusion->splat < 0 || occlusion->splat > RGBD_MAX_SPLAT)) {
        note_error(who, "occlusion: splat must be between 0 and 8");
        return nullptr;
    }
    if (occlusion && !(std::isfinite(occlusion->margin) && occlusion->margin >= 0.0)) {
        note_error(who, "occlusion: margin must be finite and not negative");
        return nullptr;
    }
    const int magnitude = depthfilter ? depthfilter->spatial_magnitude : 0;
    const bool temporal = depthfilter && depthfilter->temporal != 0;
    if (depthfilter) {
        if (magnitude < 0 || magnitude > RGBD_MAX_SPATIAL_MAGNITUDE) {
            note_error(who, "depthfilter: spatial_magnitude must be between 0 and 5");
            return nullptr;
        }
        if (depthfilter->temporal_persistency < 0 || depthfilter->temporal_persistency > RGBD_MAX_PERSISTENCY) {
            note_error(who, "depthfilter: temporal_persistency must be between 0 and 8");
            return nullptr;
        }
        if (magnitude > 0)
            if (const char *problem = smooth_problem(depthfilter->spatial_alpha, depthfilter->spatial_delta)) {
                note_error(who, std::string("depthfilter: spatial_") + problem);
                return nullptr;
            }
        if (temporal)
            if (const char *problem = smooth_problem(depthfilter->temporal_alpha, depthfilter->temporal_delta)) {
                note_error(who, std::string("depthfilter: temporal_") + problem);
                return nullptr;
            }
    }
    const int fill_mode = holefill ? holefill->mode : 0;
    if (fill_mode < 0 || fill_mode > RGBD_MAX_HOLEFILL) {
        note_error(who, "holefill: mode must be between 0 and 3");
        return nullptr;
    }
    const bool attach = (attach_flags & (CWIPC_HIP_RGBD_ATTACH_RGB | CWIPC_HIP_RGBD_ATTACH_DEPTH)) != 0;
    size_t staged_bytes = 0;
    for (int k = 0; k < ncam; k++) {
        const cwipc_hip_rgbd_sensor &s = rig->full[(size_t)k];
        if (frames[k].depth == nullptr || frames[k].colour == nullptr || (attach_flags != 0 && !rig->has_serial[(size_t)k])) {
            note_error(who, "camera " + std::to_string(k) + ": NULL argument");
            return nullptr;
        }
        const size_t depth_bytes = (size_t)s.width * (size_t)s.height * 2, colour_bytes = (size_t)s.colour_width * (size_t)s.colour_height * (size_t)s.colour_bpp;
        if (!host_range_device_alias(frames[k].depth, depth_bytes)) staged_bytes += round256(depth_bytes);
        if (!host_range_device_alias(frames[k].colour, colour_bytes)) staged_bytes += round256(colour_bytes);
    }
    if (!device_available(who)) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    if (current_device() != rig->device) {
        note_error(who, "the rig was made on another device");
        return nullptr;
    }
    std::lock_guard<std::mutex> guard(rig->lock);

    const RgbdFilterTerms f = filter_terms(filter);
    const uint32_t total = rig->total;
    const size_t nb = k::rgbd_blocks(total);
    uint8_t *stage = (uint8_t *)c.staging(staged_bytes ? staged_bytes : 256);
    uint32_t *counts = (uint32_t *)c.device_scratch((nb + 1) * sizeof(uint32_t));
    auto dst = soa_alloc((size_t)total);
    if (!stage || !counts || !dst) {
        note_error(who, "out of memory");
        return nullptr;
    }
    if (occlusion && !rig->zbuf) {   // (kept from here on: freed with the rig)
        rig->zbuf = (unsigned long long *)pool_alloc(rig->zwords * sizeof(unsigned long long));
        if (!rig->zbuf) {
            note_error(who, "out of memory");
            return nullptr;
        }
    }
    if (temporal && !rig->state) {   // (kept from here on: freed with the rig)
        rig->state = (uint8_t *)pool_alloc(round256((size_t)total * sizeof(double)) + (size_t)total);
        if (!rig->state) {
            note_error(who, "out of memory");
            return nullptr;
        }
        rig->state_empty = true;
    }
    if (fill_mode >= 2 && !rig->fill) {   // (kept from here on: freed with the rig)
        rig->fill = (uint16_t *)pool_alloc((size_t)total * sizeof(uint16_t));
        if (!rig->fill) {
            note_error(who, "out of memory");
            return nullptr;
        }
    }
    // the attached images come back into memory of their own, which the metadata then own
    std::vector<void *> images;
    struct FreeImages { std::vector<void *> &v; ~FreeImages() { for (void *p : v) ::free(p); } } free_images{images};
    if (attach)
        for (int k = 0; k < ncam; k++) {
            const size_t npix = (size_t)rig->sensors[(size_t)k].width * (size_t)rig->sensors[(size_t)k].height;
            images.push_back((attach_flags & CWIPC_HIP_RGBD_ATTACH_RGB) ? malloc(npix * 3) : nullptr);
            images.push_back((attach_flags & CWIPC_HIP_RGBD_ATTACH_DEPTH) ? malloc(npix * 2) : nullptr);
            if (((attach_flags & CWIPC_HIP_RGBD_ATTACH_RGB) && !images[images.size() - 2]) || ((attach_flags & CWIPC_HIP_RGBD_ATTACH_DEPTH) && !images.back())) {
                note_error(who, "out of memory");
                return nullptr;
            }
        }
    const k::RgbdRawCamDev *table = (const k::RgbdRawCamDev *)rig->dev;
    bool ok = true;
    for (int k = 0; k < ncam && ok; k++) {
        const cwipc_hip_rgbd_sensor &s = rig->full[(size_t)k];
        const k::RgbdRawCamDev &t = rig->table[(size_t)k];
        ok = upload(frames[k].depth, (size_t)s.width * (size_t)s.height * 2, t.full_depth ? (uint8_t *)t.full_depth : (uint8_t *)t.depth_rw, &stage, c.stream) &&
             upload(frames[k].colour, (size_t)s.colour_width * (size_t)s.colour_height * (size_t)s.colour_bpp, (uint8_t *)t.raw_colour, &stage, c.stream);
    }
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 1);
    bool cleared = true;
    if (ok && rig->decimation > 1) k::rgbd_decimate(table, ncam, rig->decimation, rig->decimate_tiles, c.stream);
    if (ok && magnitude > 0)
        k::rgbd_spatial(table, ncam, rig->row_groups, rig->col_groups, magnitude, rgbd_smooth_terms(depthfilter->spatial_alpha, depthfilter->spatial_delta),
                        c.stream);
    if (ok && temporal) {
        double *value = (double *)rig->state;
        uint8_t *history = rig->state + round256((size_t)total * sizeof(double));
        if (rig->state_empty) {   // a new state, a reset one, or one a failed grab left behind: s = 0, h = 0 everywhere
            if (profiling_enabled()) profile_begin("rgbd_history_clear", c.stream);
            cleared = hipMemsetAsync(rig->state, 0, round256((size_t)total * sizeof(double)) + (size_t)total, c.stream) == hipSuccess;
            if (profiling_enabled()) profile_end(c.stream);
        }
        k::rgbd_temporal(table, ncam, total, rgbd_smooth_terms(depthfilter->temporal_alpha, depthfilter->temporal_delta), depthfilter->temporal_persistency,
                         value, history, c.stream);
    }
    if (ok && fill_mode > 0) k::rgbd_holefill(table, ncam, fill_mode, rig->rows, total, rig->fill, c.stream);
    if (ok) {
        if (ex > 0 || ey > 0) k::rgbd_erode(table, ncam, rig->total_words, ex, ey, rig->words, c.stream);
        bool filled = true;
        if (occlusion) {
            // all ones is above every key, and a memset needs no launch; under the profiler it shows as a step of its own
            if (profiling_enabled()) profile_begin("rgbd_zfill", c.stream);
            filled = hipMemsetAsync(rig->zbuf, 0xff, rig->zwords * sizeof(unsigned long long), c.stream) == hipSuccess;
            if (profiling_enabled()) profile_end(c.stream);
            k::rgbd_zsplat(table, ncam, total, rig->zbuf, c.stream);
            k::rgbd_register_occluded(table, ncam, total, rig->zbuf, occlusion->splat, occlusion->margin, c.stream);
        } else {
            k::rgbd_register(table, ncam, total, c.stream);
        }
        k::rgbd_count(table, ncam, total, f, counts, c.tickets, report.device(), tag, c.stream);
        k::rgbd_scatter(table, ncam, total, f, counts, *dst, c.stream);
        ok = hipGetLastError() == hipSuccess && filled && cleared;
        for (int k = 0; k < ncam && ok && attach; k++) {
            const k::RgbdRawCamDev &t = rig->table[(size_t)k];
            const size_t npix = (size_t)t.width * (size_t)t.height;
            if (images[2 * (size_t)k]) ok = hipMemcpyAsync(images[2 * (size_t)k], t.registered, npix * 3, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
            if (ok && images[2 * (size_t)k + 1])
                ok = hipMemcpyAsync(images[2 * (size_t)k + 1], t.depth_rw, npix * 2, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        }
    }
    ok = c.sync() && ok;   // (also on failure: copies that read the staging buffer and kernels that write the planes may be in flight)
    if (temporal) rig->state_empty = !ok;   // (a grab that fails on the device leaves the history empty: the next one clears it)
    cwipc_hip_pointcloud *rv = finish_cloud(who, c, ok, tag, dst, rig->tiles, timestamp, cellsize);
    if (!rv) return nullptr;
    if (attach) {
        cwipc_metadata *meta = rv->access_metadata();
        for (int k = 0; k < ncam; k++) {
            const cwipc_hip_rgbd_sensor &s = rig->sensors[(size_t)k];
            const std::string size = "width=" + std::to_string(s.width) + ",height=" + std::to_string(s.height);
            const size_t npix = (size_t)s.width * (size_t)s.height;
            if (images[2 * (size_t)k]) meta->_add("rgb." + rig->serials[(size_t)k], size + ",bpp=3", images[2 * (size_t)k], npix * 3, ::free);
            if (images[2 * (size_t)k + 1]) meta->_add("depth." + rig->serials[(size_t)k], size + ",bpp=2", images[2 * (size_t)k + 1], npix * 2, ::free);
        }
        images.clear();   // (the metadata own them now)
    }
    return rv;
}

}  // namespace

extern "C" cwipc_pointcloud *cwipc_hip_rgbd_rig_grab(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_prep *prep,
                                                     const cwipc_hip_rgbd_filter *filter, uint64_t timestamp, float cellsize, int attach_flags,
                                                     char **errorMessage) {
    return rig_grab("cwipc_hip_rgbd_rig_grab", rig, frames, nullptr, nullptr, prep, nullptr, filter, timestamp, cellsize, attach_flags, errorMessage);
}

extern "C" cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_occluded(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_prep *prep,
                                                              const cwipc_hip_rgbd_occlusion *occlusion, const cwipc_hip_rgbd_filter *filter,
                                                              uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage) {
    return rig_grab("cwipc_hip_rgbd_rig_grab_occluded", rig, frames, nullptr, nullptr, prep, occlusion, filter, timestamp, cellsize, attach_flags, errorMessage);
}

extern "C" cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_filtered(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames,
                                                              const cwipc_hip_rgbd_depthfilter *depthfilter, const cwipc_hip_rgbd_prep *prep,
                                                              const cwipc_hip_rgbd_occlusion *occlusion, const cwipc_hip_rgbd_filter *filter,
                                                              uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage) {
    return rig_grab("cwipc_hip_rgbd_rig_grab_filtered", rig, frames, nullptr, depthfilter, prep, occlusion, filter, timestamp, cellsize, attach_flags, errorMessage);
}

extern "C" cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_filled(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_holefill *holefill,
                                                            const cwipc_hip_rgbd_depthfilter *depthfilter, const cwipc_hip_rgbd_prep *prep,
                                                            const cwipc_hip_rgbd_occlusion *occlusion, const cwipc_hip_rgbd_filter *filter,
                                                            uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage) {
    return rig_grab("cwipc_hip_rgbd_rig_grab_filled", rig, frames, holefill, depthfilter, prep, occlusion, filter, timestamp, cellsize, attach_flags,
                    errorMessage);
}

extern "C" void cwipc_hip_rgbd_rig_reset_history(cwipc_hip_rgbd_rig *rig) {
    if (rig == nullptr) return;
    std::lock_guard<std::mutex> guard(rig->lock);
    rig->state_empty = true;   // (no device work here: the next temporal grab clears the state before it reads it)
}

extern "C" int cwipc_hip_rgbd_rig_history(cwipc_hip_rgbd_rig *rig, int cam, double *value, uint8_t *history) {
    if (!rig_camera_ok(rig, cam) || value == nullptr || history == nullptr) return -1;
    const k::RgbdRawCamDev &t = rig->table[(size_t)cam];
    const size_t npix = (size_t)t.width * (size_t)t.height;
    std::lock_guard<std::mutex> guard(rig->lock);
    if (!rig->state || rig->state_empty) {
        memset(value, 0, npix * sizeof(double));
        memset(history, 0, npix);
        return 0;
    }
    if (!device_available("cwipc_hip_rgbd_rig_history")) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure() || current_device() != rig->device) return -1;
    bool ok = hipMemcpyAsync(value, rig->state + (size_t)t.first * sizeof(double), npix * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess &&
              hipMemcpyAsync(history, rig->state + round256((size_t)rig->total * sizeof(double)) + t.first, npix, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    return ok ? 0 : -1;
}

extern "C" const double *cwipc_hip_rgbd_rig_ray_table(const cwipc_hip_rgbd_rig *rig, int cam) {
    return rig_camera_ok(rig, cam) ? rig->rays[(size_t)cam].data() : nullptr;
}

extern "C" int cwipc_hip_rgbd_rig_grid_sensor(const cwipc_hip_rgbd_rig *rig, int cam, cwipc_hip_rgbd_sensor *out) {
    if (!rig_camera_ok(rig, cam) || out == nullptr) return -1;
    *out = rig->sensors[(size_t)cam];   // (serial is NULL in it: the caller's string was not kept)
    return 0;
}

extern "C" int cwipc_hip_rgbd_rig_map2d3d(const cwipc_hip_rgbd_rig *rig, int cam, int u, int v, int d, float out[3]) {
    if (!rig_camera_ok(rig, cam) || out == nullptr || d <= 0) return 0;
    const cwipc_hip_rgbd_sensor &s = rig->sensors[(size_t)cam];
    if (u < 0 || v < 0 || u >= s.width || v >= s.height) return 0;
    const double *ray = &rig->rays[(size_t)cam][2 * ((size_t)v * (size_t)s.width + (size_t)u)];
    if (ray[0] != ray[0] || ray[1] != ray[1]) return 0;
    rgbd_raw_point(rig->table[(size_t)cam].t, rig->table[(size_t)cam].rays ? ray : nullptr, u, v, (unsigned)d, out);
    return 1;
}

extern "C" int cwipc_hip_rgbd_rig_mapcolordepth(const cwipc_hip_rgbd_rig *rig, int cam, int u, int v, int out[2]) {
    if (!rig_camera_ok(rig, cam) || out == nullptr) return 0;
    const cwipc_hip_rgbd_sensor &s = rig->sensors[(size_t)cam];
    if (u < 0 || v < 0 || u >= s.width || v >= s.height) return 0;
    out[0] = u;
    out[1] = v;
    return 1;
}
