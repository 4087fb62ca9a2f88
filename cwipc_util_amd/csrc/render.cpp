// render.cpp -- C entry points of the renderer and the marker detector and their host orchestration (the headless coarse alignment:
// a camera's tile rendered, the markers found in the picture).  The kernels are kernels_render.hip and kernels_markers.hip.  There is
// NO CPU fallback.
#include "entry.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace cwipc_amd;

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/multicoarse.py:333-360 (the open3d window's colour and depth capture of one camera's tile)
// ---------------------------------------------------------------------------
// The argument checks of cwipc_hip_render that do not touch the cloud; false: the text has been noted.
static bool render_check_view(const char *who, const cwipc_hip_view *view, int point_size) {
    if (view->width < 1 || view->height < 1 || (int64_t)view->width * (int64_t)view->height > ((int64_t)1 << 24)) {
        note_error(who, "width and height must be at least 1 and width * height at most 2^24");
        return false;
    }
    if (point_size < 1 || point_size > 15 || (point_size & 1) == 0) {
        note_error(who, "point_size must be odd and between 1 and 15");
        return false;
    }
    bool finite = std::isfinite(view->fx) && std::isfinite(view->fy) && std::isfinite(view->cx) && std::isfinite(view->cy);
    for (int i = 0; i < 16; i++) finite = finite && std::isfinite(view->extrinsic[i]);
    if (!finite) {
        note_error(who, "the intrinsics and the extrinsic matrix must be finite");
        return false;
    }
    if (!(view->near > 0.0) || !(view->far > view->near)) {
        note_error(who, "near must be positive and far greater than near (inf: no far plane)");
        return false;
    }
    return true;
}

// The cloud of a render call on the device, nullptr (text noted) when there is none or it has too many points.
static std::shared_ptr<DeviceSoA> render_input(const char *who, cwipc_pointcloud *pc, std::unique_ptr<cwipc_hip_pointcloud> &keep) {
    auto src = device_input(who, pc, keep);
    if (!src) {
        if (!*cwipc_hip_last_error()) note_error(who, "the argument has no point data");
        return nullptr;
    }
    if (src->npoints >= 0xFFFFFFFFull) {   // (the key's low word; a cloud's count is an int anyway)
        note_error(who, "too many points");
        return nullptr;
    }
    return src;
}

// What a render leaves on the device, in one block: the count | depth | rgb | index, each part on a 16-byte boundary
struct RenderLayout {
    size_t npix, off_depth, off_rgb, off_index, bytes;
    RenderLayout(const cwipc_hip_view *view, bool with_index) {
        npix = (size_t)view->width * (size_t)view->height;
        const size_t plane = (npix * 4 + 15) & ~(size_t)15, rgb_bytes = (npix * 3 + 15) & ~(size_t)15;
        off_depth = 16; off_rgb = off_depth + plane; off_index = off_rgb + rgb_bytes;
        bytes = with_index ? off_index + plane : off_index;
    }
};

// The three render kernels on the calling thread's stream: keys (npix words) and dev (lay.bytes) are device blocks.
static void render_launch(const DeviceSoA &src, const cwipc_hip_view *view, int point_size, int tilemask, const uint8_t background[3], const RenderLayout &lay,
                          bool with_index, unsigned long long *keys, uint8_t *dev, hipStream_t stream) {
    k::RenderArgs a;
    a.width = view->width; a.height = view->height; a.half = (point_size - 1) / 2; a.tilemask = tilemask;
    a.fx = view->fx; a.fy = view->fy; a.cx = view->cx; a.cy = view->cy; a.near_z = view->near; a.far_z = view->far;
    for (int i = 0; i < 12; i++) a.e[i] = view->extrinsic[i];
    const uint32_t bg = (uint32_t)background[0] | ((uint32_t)background[1] << 8) | ((uint32_t)background[2] << 16);
    k::render_fill(keys, lay.npix, (uint32_t *)dev, stream);
    k::render_splat(src, a, keys, stream);
    k::render_resolve(keys, src.npoints ? src.rgbt() : nullptr, lay.npix, bg, (float *)(dev + lay.off_depth), dev + lay.off_rgb,
                      with_index ? (int32_t *)(dev + lay.off_index) : nullptr, (uint32_t *)dev, stream);
}

extern "C" long cwipc_hip_render(cwipc_pointcloud *pc, const cwipc_hip_view *view, int point_size, int tilemask, const uint8_t background[3], uint8_t *rgb,
                                 float *depth, int32_t *index) {
    const char *who = "cwipc_hip_render";
    if (pc == nullptr || view == nullptr || background == nullptr || rgb == nullptr || depth == nullptr) {
        note_error(who, "NULL argument");
        return -1;
    }
    if (!render_check_view(who, view, point_size)) return -1;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = render_input(who, pc, keep);
    if (!src) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const RenderLayout lay(view, index != nullptr);
    const size_t npix = lay.npix;
    unsigned long long *keys = (unsigned long long *)pool_alloc(npix * sizeof(unsigned long long));
    uint8_t *dev = (uint8_t *)pool_alloc(lay.bytes);
    uint8_t *host = (uint8_t *)c.staging(lay.bytes);
    if (!keys || !dev || !host) {
        pool_free(keys);
        pool_free(dev);
        note_error(who, "out of memory");
        return -1;
    }
    render_launch(*src, view, point_size, tilemask, background, lay, index != nullptr, keys, dev, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(host, dev, lay.bytes, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;   // (also on failure: kernels that write the blocks may still be in flight)
    pool_free(keys);
    pool_free(dev);
    if (!ok) {
        if (!*cwipc_hip_last_error()) note_error(who, "a kernel or a copy failed");
        return -1;
    }
    parallel_memcpy(depth, host + lay.off_depth, npix * sizeof(float));
    parallel_memcpy(rgb, host + lay.off_rgb, npix * 3);
    if (index) parallel_memcpy(index, host + lay.off_index, npix * sizeof(int32_t));
    uint32_t covered;
    memcpy(&covered, host, sizeof(covered));
    return (long)covered;
}

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/multicoarse.py:492-527 (cv2.aruco's detectMarkers on the captured colour image)
// ---------------------------------------------------------------------------
static const cwipc_hip_marker_params MARKER_DEFAULTS = {40, 7, 14, 2, 0};

// The image and parameter checks of the detector; *p = the parameters to use.  false: the text has been noted.
static bool marker_check(const char *who, int width, int height, const cwipc_hip_marker_params *params, cwipc_hip_marker_params *p) {
    if (width < 1 || height < 1 || width > k::MARKER_MAX_SIDE || height > k::MARKER_MAX_SIDE || (int64_t)width * (int64_t)height > ((int64_t)1 << 24)) {
        note_error(who, "width and height must be between 1 and 8192 and width * height at most 2^24");
        return false;
    }
    *p = params ? *params : MARKER_DEFAULTS;
    if (p->window_half < 1 || p->window_half > 8192) { note_error(who, "window_half must be between 1 and 8192"); return false; }
    if (p->threshold_offset < 0 || p->threshold_offset > 255) { note_error(who, "threshold_offset must be between 0 and 255"); return false; }
    if (p->min_side < 2 || p->min_side > 8192) { note_error(who, "min_side must be between 2 and 8192"); return false; }
    if (p->max_border_errors < 0 || p->max_border_errors > 24) { note_error(who, "max_border_errors must be between 0 and 24"); return false; }
    if (p->max_bit_errors < 0 || p->max_bit_errors > 25) { note_error(who, "max_bit_errors must be between 0 and 25"); return false; }
    return true;
}

// Wait for the detector's kernels, fetch the candidates' records and apply step 8 of the contract.  The return value of the entry
// points, -1 on failure.
static long marker_collect(const char *who, ThreadCtx &c, const k::MarkerWorkspace &ws, int32_t *ids, float *corners, float *corner_depth, size_t cap) {
    bool ok = ws.ok;
    ok = ok && hipMemcpyAsync(c.host_words, ws.ncand, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    std::vector<k::MarkerRecord> records;
    if (ok) {
        uint32_t n = c.host_words[0];
        if (n > ws.cap) n = ws.cap;
        if (n > 0) {
            k::MarkerRecord *host = (k::MarkerRecord *)c.staging((size_t)n * sizeof(k::MarkerRecord));
            ok = host != nullptr;
            ok = ok && hipMemcpyAsync(host, ws.records, (size_t)n * sizeof(k::MarkerRecord), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
            ok = c.sync() && ok;
            if (ok)
                for (uint32_t i = 0; i < n; i++)
                    if (host[i].id >= 0) records.push_back(host[i]);
        }
    }
    if (!ok) {
        if (!*cwipc_hip_last_error()) note_error(who, "a kernel or a copy failed");
        return -1;
    }
    // by id, the one to keep first: the largest area, then the smallest label
    std::sort(records.begin(), records.end(), [](const k::MarkerRecord &a, const k::MarkerRecord &b) {
        if (a.id != b.id) return a.id < b.id;
        if (a.area != b.area) return a.area > b.area;
        return a.label < b.label;
    });
    size_t found = 0;
    for (size_t i = 0; i < records.size(); i++) {
        if (i > 0 && records[i].id == records[i - 1].id) continue;
        if (found < cap) {
            ids[found] = records[i].id;
            for (int q = 0; q < 4; q++) {
                corners[found * 8 + 2 * q] = (float)records[i].x[q];
                corners[found * 8 + 2 * q + 1] = (float)records[i].y[q];
                if (corner_depth) corner_depth[found * 4 + q] = records[i].depth[q];
            }
        }
        found++;
    }
    return (long)found;
}

// The image to the device (through pinned memory) and the detector's kernels behind it; the dictionary is staged behind the image.
// *block: the pool block to free after the stream has been waited for.
static k::MarkerWorkspace marker_upload_and_launch(const char *who, ThreadCtx &c, const uint8_t *rgb, int width, int height, const uint32_t *dictionary,
                                                  int nmarkers, const cwipc_hip_marker_params &p, void **block) {
    k::MarkerWorkspace ws;
    const size_t npix = (size_t)width * (size_t)height;
    const size_t rgb_bytes = (npix * 3 + 255) & ~(size_t)255, dict_bytes = (size_t)nmarkers * sizeof(uint32_t);
    const size_t work_bytes = k::marker_workspace_bytes(npix, p.min_side, nmarkers);
    uint8_t *dev = (uint8_t *)pool_alloc(rgb_bytes + work_bytes);
    uint8_t *host = (uint8_t *)c.staging(rgb_bytes + dict_bytes);
    *block = dev;
    if (!dev || !host) {
        note_error(who, "out of memory");
        return ws;
    }
    parallel_memcpy(host, rgb, npix * 3);
    memcpy(host + rgb_bytes, dictionary, dict_bytes);
    if (hipMemcpyAsync(dev, host, npix * 3, hipMemcpyHostToDevice, c.stream) != hipSuccess) return ws;
    return k::marker_launch(dev, width, height, (const uint32_t *)(host + rgb_bytes), nmarkers, p, nullptr, dev + rgb_bytes, c.stream);
}

extern "C" long cwipc_hip_detect_markers(const uint8_t *rgb, int width, int height, const uint32_t *dictionary, int nmarkers,
                                         const cwipc_hip_marker_params *params, int32_t *ids, float *corners, size_t cap) {
    const char *who = "cwipc_hip_detect_markers";
    if (rgb == nullptr || dictionary == nullptr || (cap > 0 && (ids == nullptr || corners == nullptr))) {
        note_error(who, "NULL argument");
        return -1;
    }
    cwipc_hip_marker_params p;
    if (!marker_check(who, width, height, params, &p)) return -1;
    if (nmarkers < 1) {
        note_error(who, "nmarkers must be at least 1");
        return -1;
    }
    if (!device_available(who)) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    void *block = nullptr;
    const k::MarkerWorkspace ws = marker_upload_and_launch(who, c, rgb, width, height, dictionary, nmarkers, p, &block);
    const long rv = marker_collect(who, c, ws, ids, corners, nullptr, cap);   // (waits, also on failure)
    pool_free(block);
    return rv;
}

extern "C" int cwipc_hip_marker_labels(const uint8_t *rgb, int width, int height, const cwipc_hip_marker_params *params, int32_t *labels) {
    const char *who = "cwipc_hip_marker_labels";
    if (rgb == nullptr || labels == nullptr) {
        note_error(who, "NULL argument");
        return -1;
    }
    cwipc_hip_marker_params p;
    if (!marker_check(who, width, height, params, &p)) return -1;
    if (!device_available(who)) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const size_t npix = (size_t)width * (size_t)height;
    const uint32_t no_marker = 0;   // a dictionary of one word: the labels do not depend on it
    void *block = nullptr;
    int32_t *dev_out = (int32_t *)pool_alloc(npix * sizeof(int32_t));
    const k::MarkerWorkspace ws = marker_upload_and_launch(who, c, rgb, width, height, &no_marker, 1, p, &block);
    bool ok = ws.ok && dev_out != nullptr;
    if (ok) k::marker_labels_out(ws.label, npix, dev_out, c.stream);
    ok = ok && hipGetLastError() == hipSuccess;
    ok = c.sync() && ok;
    // (the staging buffer held the image until the wait; it is free for the way back now)
    int32_t *host = ok ? (int32_t *)c.staging(npix * sizeof(int32_t)) : nullptr;
    ok = ok && host != nullptr && hipMemcpyAsync(host, dev_out, npix * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(block);
    pool_free(dev_out);
    if (!ok) {
        if (!*cwipc_hip_last_error()) note_error(who, "a kernel or a copy failed");
        return -1;
    }
    parallel_memcpy(labels, host, npix * sizeof(int32_t));
    return 0;
}

extern "C" long cwipc_hip_render_detect_markers(cwipc_pointcloud *pc, const cwipc_hip_view *view, int point_size, int tilemask, const uint8_t background[3],
                                                const uint32_t *dictionary, int nmarkers, const cwipc_hip_marker_params *params, int32_t *ids,
                                                float *corners, float *corner_depth, size_t cap) {
    const char *who = "cwipc_hip_render_detect_markers";
    if (pc == nullptr || view == nullptr || background == nullptr || dictionary == nullptr || (cap > 0 && (ids == nullptr || corners == nullptr))) {
        note_error(who, "NULL argument");
        return -1;
    }
    if (!render_check_view(who, view, point_size)) return -1;
    cwipc_hip_marker_params p;
    if (!marker_check(who, view->width, view->height, params, &p)) return -1;
    if (nmarkers < 1) {
        note_error(who, "nmarkers must be at least 1");
        return -1;
    }
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = render_input(who, pc, keep);
    if (!src) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const RenderLayout lay(view, false);
    const size_t dict_bytes = (size_t)nmarkers * sizeof(uint32_t);
    unsigned long long *keys = (unsigned long long *)pool_alloc(lay.npix * sizeof(unsigned long long));
    uint8_t *dev = (uint8_t *)pool_alloc(lay.bytes);
    void *work = pool_alloc(k::marker_workspace_bytes(lay.npix, p.min_side, nmarkers));
    uint32_t *dict_host = (uint32_t *)c.staging(dict_bytes);
    if (!keys || !dev || !work || !dict_host) {
        pool_free(keys);
        pool_free(dev);
        pool_free(work);
        note_error(who, "out of memory");
        return -1;
    }
    memcpy(dict_host, dictionary, dict_bytes);
    render_launch(*src, view, point_size, tilemask, background, lay, false, keys, dev, c.stream);
    k::MarkerWorkspace ws;
    if (hipGetLastError() == hipSuccess)
        ws = k::marker_launch(dev + lay.off_rgb, view->width, view->height, dict_host, nmarkers, p, (const float *)(dev + lay.off_depth), work, c.stream);
    const long rv = marker_collect(who, c, ws, ids, corners, corner_depth, cap);   // (waits, also on failure)
    pool_free(keys);
    pool_free(dev);
    pool_free(work);
    return rv;
}
