// rgbd.cpp -- the RGB-D source end: cwipc_hip_from_rgbd builds one device-resident cloud from the cameras' depth and colour images,
// the step a capturer plug-in of the reference does on the host (its shared per-point filters: reference
// include/cwipc_util/internal/capturers.hpp:208-275).  Host orchestration only: the arithmetic is rgbd_terms.hpp's, the kernels are
// kernels_rgbd.hip's.  The images go up with asynchronous copies on the calling thread's stream (from where they lie when the caller
// holds them in page-locked memory, through the thread's pinned staging buffer otherwise) together with one small table of cameras;
// the point count comes back in a pinned word.  The two mappings a grabber answers for the registration tooling are here too, on the
// host.  There is NO CPU fallback for the cloud: without a usable GPU the call logs an ERROR and returns NULL.
#include "internal.hpp"

#include <cmath>
#include <cstring>

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

}  // namespace

extern "C" cwipc_pointcloud *cwipc_hip_from_rgbd(const cwipc_hip_rgbd_camera *cams, int ncam, const cwipc_hip_rgbd_filter *filter, uint64_t timestamp,
                                                 float cellsize, int attach_flags, char **errorMessage) {
    const char *who = "cwipc_hip_from_rgbd";
    cwipc_log_set_errorbuf(errorMessage);
    struct ErrorbufReset { ~ErrorbufReset() { cwipc_log_set_errorbuf(nullptr); } } reset;
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

    RgbdFilterTerms f{};
    if (filter) {
        f.near_z = filter->threshold_near; f.far_z = filter->threshold_far;
        f.height_min = filter->height_min; f.height_max = filter->height_max;
        f.radius = filter->radius; f.green = filter->greenscreen;
    }
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
    const uint32_t tag = ++c.tag ? c.tag : ++c.tag;
    volatile unsigned long long *word = reinterpret_cast<volatile unsigned long long *>(c.host_words);
    *word = 0ull;
    if (ok) {
        k::rgbd_count((const k::RgbdCamDev *)dev, ncam, (uint32_t)total, f, counts, c.tickets, reinterpret_cast<unsigned long long *>(c.host_words), tag, c.stream);
        k::rgbd_scatter((const k::RgbdCamDev *)dev, ncam, (uint32_t)total, f, counts, *dst, c.stream);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = c.sync() && ok;   // (also on failure: copies that read the staging buffer and kernels that write the planes may be in flight)
    pool_free(dev);
    const size_t kept = (uint32_t)*word;
    if (!ok || (uint32_t)(*word >> 32) != tag || kept > total) {
        if (ok) note_error(who, "inconsistent point count");
        else if (!*cwipc_hip_last_error()) note_error(who, "a kernel or a copy failed");
        else cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, cwipc_hip_last_error());
        return nullptr;
    }
    if (kept * 16 >= total) {
        dst->npoints = kept;   // the planes keep their spacing, only the count shrinks (as a compaction's result)
    } else {
        auto small = soa_alloc(kept);
        if (!small) return nullptr;
        if (kept) {
            bool copied = hipMemcpyAsync(small->x(), dst->x(), kept * 4, hipMemcpyDeviceToDevice, c.stream) == hipSuccess &&
                          hipMemcpyAsync(small->y(), dst->y(), kept * 4, hipMemcpyDeviceToDevice, c.stream) == hipSuccess &&
                          hipMemcpyAsync(small->z(), dst->z(), kept * 4, hipMemcpyDeviceToDevice, c.stream) == hipSuccess &&
                          hipMemcpyAsync(small->rgbt(), dst->rgbt(), kept * 4, hipMemcpyDeviceToDevice, c.stream) == hipSuccess;
            copied = c.sync() && copied;
            if (!copied) { hip_failed(hipGetLastError(), "cwipc_hip_from_rgbd", __FILE__, __LINE__); return nullptr; }
        }
        dst = small;
    }
    dst->set_tiles(tiles);
    auto *rv = new cwipc_hip_pointcloud();
    rv->adopt_device(dst, timestamp, cellsize);
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
