// rgbd.cpp -- the RGB-D source end for aligned images: cwipc_hip_from_rgbd builds one device-resident cloud from the cameras' depth and
// colour images, the step a capturer plug-in of the reference does on the host (its shared per-point filters: reference
// include/cwipc_util/internal/capturers.hpp:208-275).  Host orchestration only: the arithmetic is rgbd_terms.hpp's, the kernels are
// kernels_rgbd.hip's, the refusals and the device block's layout are rgbd_stage.hpp's.  The images go up with asynchronous copies on
// the calling thread's stream (from where they lie when the caller holds them in page-locked memory, through the thread's pinned
// staging buffer otherwise) together with one small table of cameras; the point count comes back in a pinned word.  The two mappings a
// grabber answers for the registration tooling are here too, on the host.  There is NO CPU fallback for the cloud: without a usable
// GPU the call logs an ERROR and returns NULL.  (The raw entry, cwipc_hip_rgbd_rig_*: rgbd_rig.cpp.)
#include "rgbd_shared.hpp"

using namespace cwipc_amd;

namespace {

RgbdCamTerms camera_terms(const cwipc_hip_rgbd_camera &cam) {
    RgbdCamTerms t;
    t.fx = cam.fx; t.fy = cam.fy; t.cx = cam.cx; t.cy = cam.cy; t.depth_scale = cam.depth_scale;
    for (int i = 0; i < 12; i++) t.m[i] = cam.trafo[i];
    return t;
}

// a copy of an image of the caller's, for the cloud's metadata to own
void attach_copy(cwipc_metadata *meta, const char *kind, const cwipc_hip_rgbd_camera &cam, int bpp, const void *data) {
    const size_t bytes = (size_t)cam.width * (size_t)cam.height * (size_t)bpp;
    void *copy = malloc(bytes);
    if (!copy) return;
    memcpy(copy, data, bytes);
    rgbd_attach_image(meta, kind, cam.serial, cam.width, cam.height, bpp, copy);
}

cwipc_pointcloud *from_rgbd(const char *who, const cwipc_hip_rgbd_camera *cams, int ncam, const cwipc_hip_rgbd_filter *filter, uint64_t timestamp,
                            float cellsize, int attach_flags) {
    const std::string refusal = rgbd_frame_refusal(cams, ncam, attach_flags);
    if (!refusal.empty()) {
        note_error(who, refusal);
        return nullptr;
    }
    const RgbdFrameLayout layout = rgbd_frame_layout(cams, ncam);
    size_t staged_bytes = 0;
    for (int k = 0; k < ncam; k++) {
        const RgbdFrameBytes b = rgbd_frame_bytes(cams[k]);
        staged_bytes += rgbd_staged_bytes(cams[k].depth, b.depth) + rgbd_staged_bytes(cams[k].colour, b.colour);
    }
    if (!device_available(who)) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;

    const RgbdFilterTerms f = rgbd_filter_terms(filter);
    const uint32_t total = layout.total;
    const size_t nb = k::rgbd_blocks(total);
    uint8_t *dev = (uint8_t *)pool_alloc(layout.bytes);
    uint8_t *host = (uint8_t *)c.staging(layout.table_bytes + staged_bytes);
    uint32_t *counts = (uint32_t *)c.device_scratch((nb + 1) * sizeof(uint32_t));
    auto dst = soa_alloc((size_t)total);
    if (!dev || !host || !counts || !dst) {
        pool_free(dev);
        note_error(who, "out of memory");
        return nullptr;
    }
    k::RgbdCamDev *table = (k::RgbdCamDev *)host;
    uint8_t *stage = host + layout.table_bytes;
    uint32_t tiles[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = true;
    for (int k = 0; k < ncam && ok; k++) {
        const cwipc_hip_rgbd_camera &cam = cams[k];
        const RgbdFrameLayout::Cam &part = layout.cams[(size_t)k];
        const RgbdFrameBytes b = rgbd_frame_bytes(cam);
        k::RgbdCamDev &t = table[k];
        t.t = camera_terms(cam);
        t.depth = (const uint16_t *)(dev + part.depth);
        t.colour = dev + part.colour;
        t.width = (uint32_t)cam.width; t.bpp = (uint32_t)cam.bpp; t.tile = cam.tile; t.first = part.first;
        ok = rgbd_upload(cam.depth, b.depth, dev + part.depth, &stage, c.stream) && rgbd_upload(cam.colour, b.colour, dev + part.colour, &stage, c.stream);
        tiles[cam.tile >> 5] |= 1u << (cam.tile & 31u);
    }
    ok = ok && hipMemcpyAsync(dev, table, (size_t)ncam * sizeof(k::RgbdCamDev), hipMemcpyHostToDevice, c.stream) == hipSuccess;
    // the scan publishes the point count with this tag in the upper half of the first 64-bit pinned word (as the compaction driver's)
    PinnedReport report = c.report();
    const uint32_t tag = report.arm(0, 1);
    if (ok) {
        k::rgbd_count((const k::RgbdCamDev *)dev, ncam, total, f, counts, c.tickets, report.device(), tag, c.stream);
        k::rgbd_scatter((const k::RgbdCamDev *)dev, ncam, total, f, counts, *dst, c.stream);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;   // (also on failure: copies that read the staging buffer and kernels that write the planes may be in flight)
    pool_free(dev);
    cwipc_hip_pointcloud *rv = rgbd_finish_cloud(who, c, ok, tag, dst, tiles, timestamp, cellsize);
    if (!rv) return nullptr;
    if (attach_flags & (CWIPC_HIP_RGBD_ATTACH_RGB | CWIPC_HIP_RGBD_ATTACH_DEPTH)) {
        cwipc_metadata *meta = rv->access_metadata();
        for (int k = 0; k < ncam; k++) {
            if (attach_flags & CWIPC_HIP_RGBD_ATTACH_RGB) attach_copy(meta, "rgb", cams[k], cams[k].bpp, cams[k].colour);
            if (attach_flags & CWIPC_HIP_RGBD_ATTACH_DEPTH) attach_copy(meta, "depth", cams[k], 2, cams[k].depth);
        }
    }
    return rv;
}

}  // namespace

extern "C" cwipc_pointcloud *cwipc_hip_from_rgbd(const cwipc_hip_rgbd_camera *cams, int ncam, const cwipc_hip_rgbd_filter *filter, uint64_t timestamp,
                                                 float cellsize, int attach_flags, char **errorMessage) {
    const char *who = "cwipc_hip_from_rgbd";
    ErrorbufScope errors(errorMessage);
    return guarded(who, (cwipc_pointcloud *)nullptr, [&] { return from_rgbd(who, cams, ncam, filter, timestamp, cellsize, attach_flags); });
}

extern "C" int cwipc_hip_rgbd_map2d3d(const cwipc_hip_rgbd_camera *cam, int u, int v, int d, float out[3]) {
    if (cam == nullptr || out == nullptr || d <= 0 || rgbd_camera_problem(*cam) != nullptr) return 0;
    rgbd_point(camera_terms(*cam), u, v, (unsigned)d, out);
    return 1;
}

extern "C" int cwipc_hip_rgbd_mapcolordepth(const cwipc_hip_rgbd_camera *cam, int u, int v, int out[2]) {
    if (cam == nullptr || out == nullptr || u < 0 || v < 0 || u >= cam->width || v >= cam->height) return 0;
    out[0] = u;
    out[1] = v;
    return 1;
}
