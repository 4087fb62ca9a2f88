// entry.hpp -- how the C entry points of filters.cpp, registration.cpp and render.cpp resolve their cloud arguments and wrap their
// results.  (codec_encode.cpp and exchange.cpp resolve their inputs with error semantics of their own.)
#pragma once

#include "internal.hpp"

#include <cmath>

namespace cwipc_amd {

// Resolve the argument to one of our clouds with device-resident planes.
// `keep` owns a temporary when the cloud came from another implementation.
inline std::shared_ptr<DeviceSoA> device_input(const char *who, cwipc_pointcloud *pc, std::unique_ptr<cwipc_hip_pointcloud> &keep) {
    cwipc_hip_pointcloud *ours = as_ours(pc);
    if (!ours) {
        keep = import_foreign(pc);
        ours = keep.get();
        if (!ours) {
            cwipc_log(CWIPC_LOG_LEVEL_WARNING, who, "cannot read the point data of the argument");
            return nullptr;
        }
    }
    if (!ours->has_data()) {
        // the reference sees a NULL pcl cloud here (src/cwipc_filters.cpp:37-40 and alike)
        cwipc_log(CWIPC_LOG_LEVEL_WARNING, who, "pcl_pointcloud is NULL");
        return nullptr;
    }
    if (!device_available(who)) return nullptr;
    return ours->device_points();
}

// Filters that keep coordinates and order keep the first point (the octree anchor of a later
// cwipc_downsample): no device read-back needed for it.
inline void inherit_first(DeviceSoA &dst, const DeviceSoA &src) {
    if (src.has_first && dst.npoints == src.npoints) {
        dst.first[0] = src.first[0]; dst.first[1] = src.first[1]; dst.first[2] = src.first[2];
        dst.has_first = true;
    }
}

inline cwipc_pointcloud *wrap(std::shared_ptr<DeviceSoA> planes, uint64_t timestamp, float cellsize) {
    if (!planes) return nullptr;
    auto *rv = new cwipc_hip_pointcloud();
    rv->adopt_device(planes, timestamp, cellsize);
    return rv;
}

// The same for the entry points that log a NULL cloud as an ERROR (the registration helpers).
inline std::shared_ptr<DeviceSoA> floor_input(const char *who, cwipc_pointcloud *pc, std::unique_ptr<cwipc_hip_pointcloud> &keep) {
    if (pc == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return nullptr;
    }
    return device_input(who, pc, keep);
}

// The neighbourhood arguments of the direction filter, the normals and every ICP entry that estimates normals.
inline bool direction_args_ok(const char *who, float radius, int max_nn) {
    if (radius > 0.f && std::isfinite(radius) && max_nn >= 1 && max_nn <= DIRECTION_MAX_NN) return true;
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "radius must be positive and finite, max_nn between 1 and 128");
    return false;
}

}  // namespace cwipc_amd
