// rgbd_rig.cpp -- the RGB-D source's raw entry (cwipc_hip_rgbd_rig_*, rgbd_lens.hpp): a rig keeps what is constant per camera -- the
// camera table, the ray tables (computed here at creation) and the frame's device buffers -- so that a grab uploads the images and
// nothing else.  Host orchestration only: the kernels are kernels_rgbd.hip's; what is refused, what a grab's options come to and how
// the device blocks are carved is rgbd_stage.hpp's.  The occlusion test (cwipc_hip_rgbd_rig_grab_occluded) adds a z-buffer of the
// colour grids, which the first grab that asks for it allocates.  The depth post-processing (cwipc_hip_rgbd_rig_grab_filtered,
// rgbd_depthfilter.hpp) adds the temporal filter's per-pixel state in the same way.  A decimated rig
// (cwipc_hip_rgbd_rig_create_decimated, rgbd_decimate.hpp) keeps the caller's sensors for the size of the uploads and derived ones for
// everything else; hole filling (cwipc_hip_rgbd_rig_grab_filled) adds a scratch depth plane as the z-buffer is added.
// (The aligned entry, cwipc_hip_from_rgbd: rgbd.cpp.)
#include "rgbd_shared.hpp"

#include <mutex>
#include <vector>

using namespace cwipc_amd;

struct cwipc_hip_rgbd_rig {
    int device = -1;
    std::vector<cwipc_hip_rgbd_sensor> sensors;  // on the rig's grid: the caller's when decimation == 1, else derived from them (RULE D)
    std::vector<cwipc_hip_rgbd_sensor> full;     // the caller's: the size of the depth images a grab is handed
    int decimation = 1;
    std::vector<std::string> serials;            // copies; has_serial says which sensors had one
    std::vector<bool> has_serial;
    std::vector<std::vector<double>> rays;       // per camera 2 * W * H doubles
    RgbdRigLayout layout;                        // of `dev`, with the pixel, validity-word and z-buffer-word totals
    std::vector<k::RgbdRawCamDev> table;         // the host copy of the device table
    uint8_t *dev = nullptr;                      // one pool block: the table | per camera its ray table, depth, colour and registered image | the words
    unsigned long long *words = nullptr;
    unsigned long long *zbuf = nullptr;          // the occlusion test's z-buffer: a pool block of its own, made by the first occluded grab
    uint8_t *state = nullptr;                    // the temporal filter's state (rgbd_state_layout): a pool block of its own, made by the first
                                                 // temporal grab
    bool state_empty = true;                     // the state is to be read as all zero: the next temporal grab clears it first
    uint16_t *fill = nullptr;                    // hole filling from around: a depth plane of `total` pixels, a pool block of its own, made by the
                                                 // first grab that needs it
    uint32_t rows = 0, decimate_tiles = 0;       // every camera's rows; the decimation kernel's workgroups
    uint32_t row_groups = 0, col_groups = 0;     // the spatial filter's workgroups: every camera's rows and columns in groups
    uint32_t tiles[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::mutex lock;                             // one grab at a time: the frame's device buffers are the rig's
    const k::RgbdRawCamDev *device_table() const { return (const k::RgbdRawCamDev *)dev; }
    int ncam() const { return (int)sensors.size(); }
    ~cwipc_hip_rgbd_rig() {
        pool_free(dev);
        pool_free(zbuf);
        pool_free(state);
        pool_free(fill);
    }
};

namespace {

RgbdCamTerms sensor_terms(const cwipc_hip_rgbd_sensor &s) {
    RgbdCamTerms t;
    t.fx = s.fx; t.fy = s.fy; t.cx = s.cx; t.cy = s.cy; t.depth_scale = s.depth_scale;
    for (int i = 0; i < 12; i++) t.m[i] = s.trafo[i];
    return t;
}

RgbdColourTerms colour_terms(const cwipc_hip_rgbd_sensor &s) {
    RgbdColourTerms t;
    t.fx = s.colour_fx; t.fy = s.colour_fy; t.cx = s.colour_cx; t.cy = s.colour_cy;
    t.lens = rgbd_lens_of(s.colour_coeffs);
    for (int i = 0; i < 12; i++) t.m[i] = s.depth_to_colour[i];
    t.width = s.colour_width; t.height = s.colour_height;
    return t;
}

bool rig_camera_ok(const cwipc_hip_rgbd_rig *rig, int cam) { return rig != nullptr && cam >= 0 && (size_t)cam < rig->sensors.size(); }

// cwipc_hip_rgbd_rig_create (decimation 1) and cwipc_hip_rgbd_rig_create_decimated
cwipc_hip_rgbd_rig *rig_create(const char *who, const cwipc_hip_rgbd_sensor *sensors, int ncam, int decimation) {
    const std::string refusal = rgbd_rig_refusal(sensors, ncam, decimation);
    if (!refusal.empty()) {
        note_error(who, refusal);
        return nullptr;
    }
    if (!device_available(who)) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;

    std::unique_ptr<cwipc_hip_rgbd_rig> rig(new cwipc_hip_rgbd_rig());
    rig->device = current_device();
    rig->full.assign(sensors, sensors + ncam);
    rig->decimation = decimation;
    rig->rays.resize((size_t)ncam);
    for (int k = 0; k < ncam; k++) {
        cwipc_hip_rgbd_sensor &whole = rig->full[(size_t)k];
        rig->has_serial.push_back(whole.serial != nullptr);
        rig->serials.push_back(whole.serial ? whole.serial : "");
        whole.serial = nullptr;   // (the caller's string is not kept)
        rig->sensors.push_back(rgbd_grid_sensor(whole, decimation));
        const cwipc_hip_rgbd_sensor &s = rig->sensors.back();
        const RgbdCamTerms t = sensor_terms(s);
        const RgbdLens lens = rgbd_lens_of(s.coeffs);
        std::vector<double> &rays = rig->rays[(size_t)k];
        rays.resize(2 * (size_t)s.width * (size_t)s.height);
        for (int v = 0; v < s.height; v++)
            for (int u = 0; u < s.width; u++) rgbd_ray(t, lens, u, v, &rays[2 * ((size_t)v * (size_t)s.width + (size_t)u)]);
        rig->tiles[s.tile >> 5] |= 1u << (s.tile & 31u);
    }
    const RgbdRigLayout &layout = rig->layout = rgbd_rig_layout(rig->sensors.data(), rig->full.data(), ncam, decimation);
    rig->dev = (uint8_t *)pool_alloc(layout.bytes);
    if (!rig->dev) {
        note_error(who, "out of memory");
        return nullptr;
    }
    uint8_t *dev = rig->dev;
    rig->words = (unsigned long long *)(dev + layout.words);
    rig->table.resize((size_t)ncam);
    bool ok = true;
    for (int k = 0; k < ncam; k++) {
        const cwipc_hip_rgbd_sensor &s = rig->sensors[(size_t)k];
        const RgbdRigLayout::Cam &part = layout.cams[(size_t)k];
        k::RgbdRawCamDev &t = rig->table[(size_t)k];
        t.t = sensor_terms(s);
        t.ct = colour_terms(s);
        t.rays = part.rays ? (const double *)(dev + part.rays) : nullptr;
        if (part.rays)
            ok = ok && hipMemcpyAsync(dev + part.rays, rig->rays[(size_t)k].data(), rig->rays[(size_t)k].size() * sizeof(double), hipMemcpyHostToDevice,
                                      c.stream) == hipSuccess;
        t.depth_rw = (uint16_t *)(dev + part.depth); t.depth = t.depth_rw;
        t.raw_colour = dev + part.raw_colour;
        t.registered = dev + part.registered; t.colour = t.registered;
        t.full_depth = part.full_depth ? (const uint16_t *)(dev + part.full_depth) : nullptr;
        t.full_width = part.full_depth ? (uint32_t)rig->full[(size_t)k].width : 0;
        t.width = (uint32_t)s.width; t.height = (uint32_t)s.height; t.bpp = 3u; t.raw_bpp = (uint32_t)s.colour_bpp; t.tile = s.tile;
        t.first = part.first; t.wpr = part.wpr; t.wfirst = part.wfirst; t.zfirst = part.zfirst;
        rig->row_groups += k::rgbd_line_groups(t.height);
        rig->col_groups += k::rgbd_line_groups(t.width);
        rig->rows += t.height;
        rig->decimate_tiles += k::rgbd_decimate_tiles(t.width, t.height);
    }
    ok = ok && hipMemcpyAsync(dev, rig->table.data(), (size_t)ncam * sizeof(k::RgbdRawCamDev), hipMemcpyHostToDevice, c.stream) == hipSuccess;
    ok = c.sync() && ok;   // (the copies read the rig's vectors: they stay, but the next call may come from another thread)
    if (!ok) {
        if (!*cwipc_hip_last_error()) note_error(who, "a copy failed");
        else cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, cwipc_hip_last_error());
        return nullptr;
    }
    return rig.release();
}

cwipc_hip_rgbd_rig *create_entry(const char *who, const cwipc_hip_rgbd_sensor *sensors, int ncam, int decimation, char **errorMessage) {
    ErrorbufScope errors(errorMessage);
    return guarded(who, (cwipc_hip_rgbd_rig *)nullptr, [&] { return rig_create(who, sensors, ncam, decimation); });
}

}  // namespace

extern "C" cwipc_hip_rgbd_rig *cwipc_hip_rgbd_rig_create(const cwipc_hip_rgbd_sensor *sensors, int ncam, char **errorMessage) {
    return create_entry("cwipc_hip_rgbd_rig_create", sensors, ncam, 1, errorMessage);
}

extern "C" cwipc_hip_rgbd_rig *cwipc_hip_rgbd_rig_create_decimated(const cwipc_hip_rgbd_sensor *sensors, int ncam, int decimation, char **errorMessage) {
    return create_entry("cwipc_hip_rgbd_rig_create_decimated", sensors, ncam, decimation, errorMessage);
}

extern "C" int cwipc_hip_rgbd_rig_decimation(const cwipc_hip_rgbd_rig *rig) { return rig ? rig->decimation : 0; }

extern "C" void cwipc_hip_rgbd_rig_free(cwipc_hip_rgbd_rig *rig) { delete rig; }

namespace {

// The images a grab attaches come back into memory of their own, which the cloud's metadata then own.
struct AttachedImages {
    struct Cam { void *rgb = nullptr, *depth = nullptr; };
    std::vector<Cam> cams;   // empty: nothing is attached
    ~AttachedImages() {
        for (Cam &cam : cams) { ::free(cam.rgb); ::free(cam.depth); }
    }
    // room for what attach_flags asks for of every camera; false: out of memory
    bool alloc(const cwipc_hip_rgbd_rig &rig, int attach_flags) {
        if (!(attach_flags & (CWIPC_HIP_RGBD_ATTACH_RGB | CWIPC_HIP_RGBD_ATTACH_DEPTH))) return true;
        cams.resize(rig.sensors.size());
        for (size_t k = 0; k < cams.size(); k++) {
            const size_t npix = (size_t)rig.sensors[k].width * (size_t)rig.sensors[k].height;
            if (attach_flags & CWIPC_HIP_RGBD_ATTACH_RGB) cams[k].rgb = malloc(npix * 3);
            if (attach_flags & CWIPC_HIP_RGBD_ATTACH_DEPTH) cams[k].depth = malloc(npix * 2);
            if (((attach_flags & CWIPC_HIP_RGBD_ATTACH_RGB) && !cams[k].rgb) || ((attach_flags & CWIPC_HIP_RGBD_ATTACH_DEPTH) && !cams[k].depth)) return false;
        }
        return true;
    }
};

// ---- the steps of a grab, in the order of the contract in hip_ext.h ----

// 1. what the plan needs and the rig does not have yet: kept from here on, freed with the rig.  false: out of memory
bool grab_resources(cwipc_hip_rgbd_rig &rig, const RgbdGrabPlan &plan) {
    if (plan.occluded && !rig.zbuf) {
        rig.zbuf = (unsigned long long *)pool_alloc(rig.layout.zwords * sizeof(unsigned long long));
        if (!rig.zbuf) return false;
    }
    if (plan.temporal && !rig.state) {
        rig.state = (uint8_t *)pool_alloc(rgbd_state_layout(rig.layout.total).bytes);
        if (!rig.state) return false;
        rig.state_empty = true;
    }
    if (plan.fill_mode >= 2 && !rig.fill) {
        rig.fill = (uint16_t *)pool_alloc((size_t)rig.layout.total * sizeof(uint16_t));
        if (!rig.fill) return false;
    }
    return true;
}

// 2. the frame's images: the depth image to the full-size plane of a decimated rig, else to the depth plane itself
bool grab_upload(const cwipc_hip_rgbd_rig &rig, const cwipc_hip_rgbd_frame *frames, uint8_t *stage, hipStream_t stream) {
    bool ok = true;
    for (size_t k = 0; k < rig.full.size() && ok; k++) {
        const RgbdFrameBytes b = rgbd_frame_bytes(rig.full[k]);
        const k::RgbdRawCamDev &t = rig.table[k];
        ok = rgbd_upload(frames[k].depth, b.depth, t.full_depth ? (uint8_t *)t.full_depth : (uint8_t *)t.depth_rw, &stage, stream) &&
             rgbd_upload(frames[k].colour, b.colour, (uint8_t *)t.raw_colour, &stage, stream);
    }
    return ok;
}

// 3. RULE D, rules 0a - 0c and rule 1 on the depth planes.  false: the clearing of the state could not be queued
bool grab_depth_stages(cwipc_hip_rgbd_rig &rig, const RgbdGrabPlan &plan, hipStream_t stream) {
    const k::RgbdRawCamDev *table = rig.device_table();
    const int ncam = rig.ncam();
    const uint32_t total = rig.layout.total;
    bool cleared = true;
    if (rig.decimation > 1) k::rgbd_decimate(table, ncam, rig.decimation, rig.decimate_tiles, stream);
    if (plan.magnitude > 0) k::rgbd_spatial(table, ncam, rig.row_groups, rig.col_groups, plan.magnitude, plan.spatial, stream);
    if (plan.temporal) {
        const RgbdStateLayout state = rgbd_state_layout(total);
        if (rig.state_empty) {   // a new state, a reset one, or one a failed grab left behind: s = 0, h = 0 everywhere
            if (profiling_enabled()) profile_begin("rgbd_history_clear", stream);
            cleared = hipMemsetAsync(rig.state, 0, state.bytes, stream) == hipSuccess;
            if (profiling_enabled()) profile_end(stream);
        }
        k::rgbd_temporal(table, ncam, total, plan.temporal_terms, plan.persistency, (double *)rig.state, rig.state + state.history, stream);
    }
    if (plan.fill_mode > 0) k::rgbd_holefill(table, ncam, plan.fill_mode, rig.rows, total, rig.fill, stream);
    if (plan.ex > 0 || plan.ey > 0) k::rgbd_erode(table, ncam, rig.layout.total_words, plan.ex, plan.ey, rig.words, stream);
    return cleared;
}

// 4. every depth pixel's colour, with rules 3a and 3b when the plan asks for them.  false: the z-buffer's fill could not be queued
bool grab_register(cwipc_hip_rgbd_rig &rig, const RgbdGrabPlan &plan, hipStream_t stream) {
    const k::RgbdRawCamDev *table = rig.device_table();
    const int ncam = rig.ncam();
    if (!plan.occluded) {
        k::rgbd_register(table, ncam, rig.layout.total, stream);
        return true;
    }
    // all ones is above every key, and a memset needs no launch; under the profiler it shows as a step of its own
    if (profiling_enabled()) profile_begin("rgbd_zfill", stream);
    const bool filled = hipMemsetAsync(rig.zbuf, 0xff, rig.layout.zwords * sizeof(unsigned long long), stream) == hipSuccess;
    if (profiling_enabled()) profile_end(stream);
    k::rgbd_zsplat(table, ncam, rig.layout.total, rig.zbuf, stream);
    k::rgbd_register_occluded(table, ncam, rig.layout.total, rig.zbuf, plan.splat, plan.margin, stream);
    return filled;
}

// 5. rule 4: the point count under `tag` into the pinned report, the points into dst
void grab_count_scatter(const cwipc_hip_rgbd_rig &rig, const RgbdFilterTerms &f, uint32_t *counts, ThreadCtx &c, PinnedReport &report, uint32_t tag,
                        const DeviceSoA &dst) {
    const k::RgbdRawCamDev *table = rig.device_table();
    const int ncam = rig.ncam();
    k::rgbd_count(table, ncam, rig.layout.total, f, counts, c.tickets, report.device(), tag, c.stream);
    k::rgbd_scatter(table, ncam, rig.layout.total, f, counts, dst, c.stream);
}

// 6. the registered and the depth images as the cloud was made from them, into the memory `images` holds
bool grab_read_back(const cwipc_hip_rgbd_rig &rig, const AttachedImages &images, hipStream_t stream) {
    bool ok = true;
    for (size_t k = 0; k < images.cams.size() && ok; k++) {
        const k::RgbdRawCamDev &t = rig.table[k];
        const size_t npix = (size_t)t.width * (size_t)t.height;
        if (images.cams[k].rgb) ok = hipMemcpyAsync(images.cams[k].rgb, t.registered, npix * 3, hipMemcpyDeviceToHost, stream) == hipSuccess;
        if (ok && images.cams[k].depth) ok = hipMemcpyAsync(images.cams[k].depth, t.depth_rw, npix * 2, hipMemcpyDeviceToHost, stream) == hipSuccess;
    }
    return ok;
}

// 7. the images become the cloud's, per camera rgb then depth
void grab_attach(const cwipc_hip_rgbd_rig &rig, AttachedImages &images, cwipc_hip_pointcloud *cloud) {
    if (images.cams.empty()) return;
    cwipc_metadata *meta = cloud->access_metadata();
    for (size_t k = 0; k < images.cams.size(); k++) {
        const cwipc_hip_rgbd_sensor &s = rig.sensors[k];
        AttachedImages::Cam &cam = images.cams[k];
        if (cam.rgb) rgbd_attach_image(meta, "rgb", rig.serials[k], s.width, s.height, 3, cam.rgb);
        cam.rgb = nullptr;   // (the metadata own it now)
        if (cam.depth) rgbd_attach_image(meta, "depth", rig.serials[k], s.width, s.height, 2, cam.depth);
        cam.depth = nullptr;
    }
}

// One flow for the four grab entries: what they differ in is the plan.
cwipc_pointcloud *rig_grab(const char *who, cwipc_hip_rgbd_rig &rig, const cwipc_hip_rgbd_frame *frames, const RgbdGrabPlan &plan,
                           const cwipc_hip_rgbd_filter *filter, uint64_t timestamp, float cellsize, int attach_flags) {
    size_t staged_bytes = 0;
    for (size_t k = 0; k < rig.full.size(); k++) {
        if (frames[k].depth == nullptr || frames[k].colour == nullptr || (attach_flags != 0 && !rig.has_serial[k])) {
            note_error(who, "camera " + std::to_string(k) + ": NULL argument");
            return nullptr;
        }
        const RgbdFrameBytes b = rgbd_frame_bytes(rig.full[k]);
        staged_bytes += rgbd_staged_bytes(frames[k].depth, b.depth) + rgbd_staged_bytes(frames[k].colour, b.colour);
    }
    if (!device_available(who)) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    if (current_device() != rig.device) {
        note_error(who, "the rig was made on another device");
        return nullptr;
    }
    std::lock_guard<std::mutex> guard(rig.lock);

    const RgbdFilterTerms f = rgbd_filter_terms(filter);
    uint8_t *stage = (uint8_t *)c.staging(staged_bytes ? staged_bytes : 256);
    uint32_t *counts = (uint32_t *)c.device_scratch((k::rgbd_blocks(rig.layout.total) + 1) * sizeof(uint32_t));
    auto dst = soa_alloc((size_t)rig.layout.total);
    AttachedImages images;
    if (!stage || !counts || !dst || !grab_resources(rig, plan) || !images.alloc(rig, attach_flags)) {
        note_error(who, "out of memory");
        return nullptr;
    }
    bool ok = grab_upload(rig, frames, stage, c.stream);
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 1);
    if (ok) {
        const bool cleared = grab_depth_stages(rig, plan, c.stream);
        const bool filled = grab_register(rig, plan, c.stream);
        grab_count_scatter(rig, f, counts, c, report, tag, *dst);
        ok = hipGetLastError() == hipSuccess && filled && cleared;
        ok = ok && grab_read_back(rig, images, c.stream);
    }
    ok = c.sync() && ok;   // (also on failure: copies that read the staging buffer and kernels that write the planes may be in flight)
    if (plan.temporal) rig.state_empty = !ok;   // (a grab that fails on the device leaves the history empty: the next one clears it)
    cwipc_hip_pointcloud *rv = rgbd_finish_cloud(who, c, ok, tag, dst, rig.tiles, timestamp, cellsize);
    if (rv) grab_attach(rig, images, rv);
    return rv;
}

// cwipc_hip_rgbd_rig_grab (no struct but prep), _grab_occluded (occlusion too), _grab_filtered (depthfilter too) and _grab_filled (all four)
cwipc_pointcloud *grab_entry(const char *who, cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_holefill *holefill,
                             const cwipc_hip_rgbd_depthfilter *depthfilter, const cwipc_hip_rgbd_prep *prep, const cwipc_hip_rgbd_occlusion *occlusion,
                             const cwipc_hip_rgbd_filter *filter, uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage) {
    ErrorbufScope errors(errorMessage);
    return guarded(who, (cwipc_pointcloud *)nullptr, [&]() -> cwipc_pointcloud * {
        RgbdGrabPlan plan;
        const std::string problem = rig == nullptr || frames == nullptr ? "NULL argument" : rgbd_grab_plan(holefill, depthfilter, prep, occlusion, plan);
        if (!problem.empty()) {
            note_error(who, problem);
            return nullptr;
        }
        return rig_grab(who, *rig, frames, plan, filter, timestamp, cellsize, attach_flags);
    });
}

}  // namespace

extern "C" cwipc_pointcloud *cwipc_hip_rgbd_rig_grab(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_prep *prep,
                                                     const cwipc_hip_rgbd_filter *filter, uint64_t timestamp, float cellsize, int attach_flags,
                                                     char **errorMessage) {
    return grab_entry("cwipc_hip_rgbd_rig_grab", rig, frames, nullptr, nullptr, prep, nullptr, filter, timestamp, cellsize, attach_flags, errorMessage);
}

extern "C" cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_occluded(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_prep *prep,
                                                              const cwipc_hip_rgbd_occlusion *occlusion, const cwipc_hip_rgbd_filter *filter,
                                                              uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage) {
    return grab_entry("cwipc_hip_rgbd_rig_grab_occluded", rig, frames, nullptr, nullptr, prep, occlusion, filter, timestamp, cellsize, attach_flags, errorMessage);
}

extern "C" cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_filtered(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames,
                                                              const cwipc_hip_rgbd_depthfilter *depthfilter, const cwipc_hip_rgbd_prep *prep,
                                                              const cwipc_hip_rgbd_occlusion *occlusion, const cwipc_hip_rgbd_filter *filter,
                                                              uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage) {
    return grab_entry("cwipc_hip_rgbd_rig_grab_filtered", rig, frames, nullptr, depthfilter, prep, occlusion, filter, timestamp, cellsize, attach_flags, errorMessage);
}

extern "C" cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_filled(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_holefill *holefill,
                                                            const cwipc_hip_rgbd_depthfilter *depthfilter, const cwipc_hip_rgbd_prep *prep,
                                                            const cwipc_hip_rgbd_occlusion *occlusion, const cwipc_hip_rgbd_filter *filter,
                                                            uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage) {
    return grab_entry("cwipc_hip_rgbd_rig_grab_filled", rig, frames, holefill, depthfilter, prep, occlusion, filter, timestamp, cellsize, attach_flags,
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
    const RgbdStateLayout state = rgbd_state_layout(rig->layout.total);
    bool ok = hipMemcpyAsync(value, rig->state + state.value_at(t.first), npix * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess &&
              hipMemcpyAsync(history, rig->state + state.history_at(t.first), npix, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
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
