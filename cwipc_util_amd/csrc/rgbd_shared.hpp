// rgbd_shared.hpp -- what the RGB-D source's aligned entry (rgbd.cpp) and its raw entry (rgbd_rig.cpp) share on the host: the way an
// image goes up, the filter's terms, the cloud a finished call hands out and the images attached to it.  (The staging arithmetic:
// rgbd_stage.hpp, through internal.hpp.)
#pragma once

#include "internal.hpp"
#include "c_boundary.hpp"

#include <cstring>
#include <string>

namespace cwipc_amd {

// An image of `bytes` at src goes up from where it lies when the caller holds it in page-locked memory, through the calling thread's
// staging buffer otherwise: the room it takes there.
inline size_t rgbd_staged_bytes(const void *src, size_t bytes) { return host_range_device_alias(src, bytes) ? 0 : stage_round256(bytes); }

// ... and its way to dev; the staging buffer at *stage moves on by that room
inline bool rgbd_upload(const void *src, size_t bytes, uint8_t *dev, uint8_t **stage, hipStream_t stream) {
    const void *from = src;
    if (const size_t room = rgbd_staged_bytes(src, bytes)) {
        parallel_memcpy(*stage, src, bytes);
        from = *stage;
        *stage += room;
    }
    return hipMemcpyAsync(dev, from, bytes, hipMemcpyHostToDevice, stream) == hipSuccess;
}

inline RgbdFilterTerms rgbd_filter_terms(const cwipc_hip_rgbd_filter *filter) {
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
inline cwipc_hip_pointcloud *rgbd_finish_cloud(const char *who, ThreadCtx &c, bool ok, uint32_t tag, std::shared_ptr<DeviceSoA> dst, const uint32_t tiles[8],
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

// `data` (malloc'ed, width x height pixels of bpp bytes) becomes the cloud's "<kind>.<serial>" image: the metadata own it from here on
inline void rgbd_attach_image(cwipc_metadata *meta, const char *kind, const std::string &serial, int width, int height, int bpp, void *data) {
    meta->_add(kind + ("." + serial), "width=" + std::to_string(width) + ",height=" + std::to_string(height) + ",bpp=" + std::to_string(bpp), data,
               (size_t)width * (size_t)height * (size_t)bpp, ::free);
}

}  // namespace cwipc_amd
