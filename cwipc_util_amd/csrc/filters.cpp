// filters.cpp -- C entry points of the per-point filter hot path and their host
// orchestration.  Reference: src/cwipc_filters.cpp (wrapping logic, NULL/ERROR
// conventions, timestamp/cellsize propagation) -- the per-point work itself is in
// kernels_*.hip.  There is NO CPU fallback: without a usable GPU every filter
// logs an ERROR and returns NULL.
#include "internal.hpp"

#include <atomic>
#include <chrono>
#include <cmath>

#include <algorithm>
#include <cstring>

namespace cwipc_amd {

namespace {

// Resolve the argument to one of our clouds with device-resident planes.
// `keep` owns a temporary when the cloud came from another implementation.
std::shared_ptr<DeviceSoA> device_input(const char *who, cwipc_pointcloud *pc, std::unique_ptr<cwipc_hip_pointcloud> &keep) {
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
void inherit_first(DeviceSoA &dst, const DeviceSoA &src) {
    if (src.has_first && dst.npoints == src.npoints) {
        dst.first[0] = src.first[0]; dst.first[1] = src.first[1]; dst.first[2] = src.first[2];
        dst.has_first = true;
    }
}

cwipc_pointcloud *wrap(std::shared_ptr<DeviceSoA> planes, uint64_t timestamp, float cellsize) {
    if (!planes) return nullptr;
    auto *rv = new cwipc_hip_pointcloud();
    rv->adopt_device(planes, timestamp, cellsize);
    return rv;
}

}  // namespace

// Stable compaction driver: count -> scan -> scatter, back to back with one wait at the end.  The
// output planes have room for every input point (the kept count is known only when the kernels are
// done; the scan kernel writes it into the thread's pinned words); a result that uses less than a
// sixteenth of that room is copied into a buffer of its own size.
std::shared_ptr<DeviceSoA> compact(const DeviceSoA &src, const k::Predicate &p, bool may_return_early) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    size_t n = src.npoints;
    if (n == 0) return soa_alloc(0);
    size_t nb = k::compact_blocks(n);
    uint32_t *counts = (uint32_t *)c.device_scratch((nb + 1) * sizeof(uint32_t));   // (+ the total, for the scatter kernel)
    auto dst = soa_alloc(n);
    if (!counts || !dst) return nullptr;
    // the scan kernel publishes the kept count with this tag in the upper half of the first 64-bit pinned word
    const uint32_t tag = ++c.tag ? c.tag : ++c.tag;
    volatile unsigned long long *word = reinterpret_cast<volatile unsigned long long *>(c.host_words);
    *word = 0ull;
    if (k::compact_count_scan(src, p, counts, c.tickets, reinterpret_cast<unsigned long long *>(c.host_words), tag, c.stream)) {
        k::compact_scatter(src, p, counts, *dst, c.stream);
    } else {
        // big clouds (r4): two launches, not three -- the scatter kernel's workgroups add up the counts in front of them themselves
        k::compact_count(src, p, counts, c.stream);
        k::compact_scatter(src, p, counts, *dst, c.stream, reinterpret_cast<unsigned long long *>(c.host_words), tag);
    }
    bool ok = hipGetLastError() == hipSuccess;
    // The count is there when the scan kernel is done; the scatter kernel behind it needs no more attention
    // from the host, so a caller that allows it gets the result back with that kernel still running.
    bool seen = false;
    if (ok && may_return_early && !profiling_enabled()) {
        const auto t_give_up = std::chrono::steady_clock::now() + std::chrono::microseconds(poll_budget_us());
        for (int spin = 0;; spin++) {
            if ((uint32_t)(*word >> 32) == tag) { seen = true; break; }
            if ((spin & 255) == 255 && std::chrono::steady_clock::now() > t_give_up) break;
            __builtin_ia32_pause();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!seen) ok = c.sync() && ok;
    if (!ok || (uint32_t)(*word >> 32) != tag) {
        (void)c.sync();   // `dst` goes back to the pool: nothing may still be writing it
        hip_failed(hipGetLastError(), "compaction", __FILE__, __LINE__);
        return nullptr;
    }
    const size_t kept = (uint32_t)*word;
    if (kept > n) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip", "compaction: inconsistent count");
        if (seen) (void)c.sync();
        return nullptr;
    }
    if (kept == n) {
        // every point kept: the result holds the input's planes (clouds are immutable); the scatter kernel saw the same total
        // and copied nothing.  (The input is complete: the count kernel, ordered behind its producer, has run.)
        auto same = std::make_shared<DeviceSoA>();
        same->xyz_block = src.xyz_block;
        same->rgbt_block = src.rgbt_block;
        same->npoints = src.npoints;
        same->stride = src.stride;
        same->device = src.device;
        if (src.has_first) { same->first[0] = src.first[0]; same->first[1] = src.first[1]; same->first[2] = src.first[2]; same->has_first = true; }
        // (`dst` goes back to the pool untouched: the scatter kernel writes nothing)
        return same;
    }
    if (kept * 16 >= n) {
        dst->npoints = kept;   // the planes keep their spacing (stride), only the count shrinks
        if (seen) {
            dst->mark_pending(c.stream);
            src.note_reader(c.stream);   // the scatter kernel is still reading the input
        }
        return dst;
    }
    if (seen && !c.sync()) return nullptr;   // the copy below reads what the scatter kernel writes, then `dst` goes back to the pool
    auto small = soa_alloc(kept);
    if (!small) return nullptr;
    if (kept) {
        bool copied = hipMemcpyAsync(small->x(), dst->x(), kept * 4, hipMemcpyDeviceToDevice, c.stream) == hipSuccess &&
                      hipMemcpyAsync(small->y(), dst->y(), kept * 4, hipMemcpyDeviceToDevice, c.stream) == hipSuccess &&
                      hipMemcpyAsync(small->z(), dst->z(), kept * 4, hipMemcpyDeviceToDevice, c.stream) == hipSuccess &&
                      hipMemcpyAsync(small->rgbt(), dst->rgbt(), kept * 4, hipMemcpyDeviceToDevice, c.stream) == hipSuccess;
        copied = c.sync() && copied;
        if (!copied) { hip_failed(hipGetLastError(), "compaction", __FILE__, __LINE__); return nullptr; }
    }
    return small;
}

}  // namespace cwipc_amd

using namespace cwipc_amd;

// ---------------------------------------------------------------------------
// reference src/cwipc_filters.cpp:281-306
// ---------------------------------------------------------------------------
extern "C" cwipc_pointcloud *cwipc_tilefilter(cwipc_pointcloud *pc, int tile) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_tilefilter", pc, keep);
    if (!src) return nullptr;
    // tile 0 keeps every point (reference :296): the result is the same cloud -- clouds are immutable, so it holds
    // the very same planes instead of a copy of them
    if (tile == 0) return wrap(src, pc->timestamp(), pc->cellsize());
    // what is known about the cloud's tiles without looking at a point (DeviceSoA::tiles): a camera's own tile through its own
    // filter -- the per-tile chain of the reference's registration tooling -- is the cloud itself; a tile that cannot occur is empty
    if (src->npoints && src->only_tile((unsigned)tile)) return wrap(src, pc->timestamp(), pc->cellsize());
    if (src->npoints && !src->may_have_tile((unsigned)tile)) {
        auto none = soa_alloc(0);
        if (none) none->set_one_tile((unsigned)tile);
        return wrap(none, pc->timestamp(), pc->cellsize());
    }
    k::Predicate p{};
    p.mode = 0;
    p.tile = tile;
    auto dst = compact(*src, p, true);
    if (dst) dst->set_one_tile((unsigned)tile);   // (tile > 255 keeps nothing, reference :296; a set of "value 255 & ..." never matters for an empty cloud)
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference python/cwipc/registration/util.py:98-112 (numpy boolean-mask selection)
extern "C" cwipc_pointcloud *cwipc_hip_tilefilter_masked(cwipc_pointcloud *pc, int mask) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_tilefilter_masked", pc, keep);
    if (!src) return nullptr;
    k::Predicate p{};
    p.mode = 2;
    p.tile = mask & 0xff;
    auto dst = compact(*src, p, true);
    if (dst) dst->set_tiles_from(*src);   // (a subset of the points: what could not occur still cannot)
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference src/cwipc_filters.cpp:333-360
extern "C" cwipc_pointcloud *cwipc_crop(cwipc_pointcloud *pc, float bbox[6]) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_crop", pc, keep);
    if (!src) return nullptr;
    k::Predicate p{};
    p.mode = 1;
    memcpy(p.bbox, bbox, 6 * sizeof(float));
    auto dst = compact(*src, p, true);
    if (dst) dst->set_tiles_from(*src);   // (a subset of the points: what could not occur still cannot)
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference src/cwipc_filters.cpp:308-331
extern "C" cwipc_pointcloud *cwipc_tilemap(cwipc_pointcloud *pc, uint8_t map[256]) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_tilemap", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_rgbt(src);   // the coordinates do not change: the result holds the very same planes
    if (!dst) return nullptr;
    // the 256-byte table travels through the per-thread pinned words
    memcpy(c.host_words, map, 256);
    bool ok = hipMemcpyAsync(c.dev_words, c.host_words, 256, hipMemcpyHostToDevice, c.stream) == hipSuccess;
    if (ok) k::map_tile(*src, *dst, (const uint8_t *)c.dev_words, c.stream);
    ok = c.sync() && ok;
    if (!ok) return nullptr;
    inherit_first(*dst, *src);
    {   // the tiles that may occur afterwards: the images of those that may occur now (of all 256 values if nothing is known)
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (unsigned t = 0; t < 256; t++)
            if (src->may_have_tile(t)) w[map[t] >> 5] |= 1u << (map[t] & 31u);
        dst->set_tiles(w);
    }
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference src/cwipc_filters.cpp:362-386
extern "C" cwipc_pointcloud *cwipc_colormap(cwipc_pointcloud *pc, uint32_t clearBits, uint32_t setBits) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_colormap", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_rgbt(src);   // the coordinates do not change: the result holds the very same planes
    if (!dst) return nullptr;
    k::map_color_bits(*src, *dst, clearBits, setBits, c.stream);
    if (!c.sync()) return nullptr;
    inherit_first(*dst, *src);
    if (src->has_tiles) {   // the tile is bits 24-31 of the word the masks work on (:377-378)
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (unsigned t = 0; t < 256; t++)
            if (src->may_have_tile(t)) { const unsigned u = ((t & ~(clearBits >> 24)) | (setBits >> 24)) & 255u; w[u >> 5] |= 1u << (u & 31u); }
        dst->set_tiles(w);
    }
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference python/cwipc/registration/util.py:295-309 (cwipc_transform: numpy R @ p + t in float64, stored as float32)
extern "C" cwipc_pointcloud *cwipc_hip_transform(cwipc_pointcloud *pc, const double *matrix4x4) {
    if (pc == nullptr || matrix4x4 == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_transform", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_xyz(src);   // colours and tiles do not change: the result holds the very same words
    if (!dst) return nullptr;
    double m[12];
    for (int r = 0; r < 3; r++)
        for (int col = 0; col < 4; col++) m[r * 4 + col] = matrix4x4[r * 4 + col];
    k::map_affine(*src, *dst, m, 0, c.stream);
    if (!c.sync()) return nullptr;
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference python/cwipc/registration/multicamera.py:399-403 (MultiCameraToFloor._prepare_floor: every point projected onto y = 0): a copy
// of the x and z planes and a memset of the y plane (+0.0 is all zero bytes), colours and tiles shared with the input.  Timestamp 0,
// cellsize 0, as cwipc_from_numpy_matrix(matrix, 0) gives them there.
extern "C" cwipc_pointcloud *cwipc_hip_flatten_y(cwipc_pointcloud *pc) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_flatten_y", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_xyz(src);
    if (!dst) return nullptr;
    const size_t plane = src->stride * sizeof(float);
    bool ok = true;
    if (plane) {
        ok = hipMemcpyAsync(dst->x(), src->x(), plane, hipMemcpyDeviceToDevice, c.stream) == hipSuccess &&
             hipMemsetAsync(dst->y(), 0, plane, c.stream) == hipSuccess &&
             hipMemcpyAsync(dst->z(), src->z(), plane, hipMemcpyDeviceToDevice, c.stream) == hipSuccess;
    }
    ok = c.sync() && ok;
    if (!ok) return nullptr;
    return wrap(dst, 0, 0.f);
}

// reference python/cwipc/filters/transform.py:38-52 (TransformFilter: (p + offset) * scale in Python floats; cellsize * scale)
extern "C" cwipc_pointcloud *cwipc_hip_offset_scale(cwipc_pointcloud *pc, double x, double y, double z, double scale) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_offset_scale", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_xyz(src);   // colours and tiles do not change: the result holds the very same words
    if (!dst) return nullptr;
    double m[12] = {scale, 0, 0, x, 0, 0, 0, y, 0, 0, 0, z};
    k::map_affine(*src, *dst, m, 1, c.stream);
    if (!c.sync()) return nullptr;
    return wrap(dst, pc->timestamp(), (float)((double)pc->cellsize() * scale));
}

// reference python/cwipc/registration/util.py:285-293 (get_tiles_used): used[t] = 1 for every tile value that occurs
extern "C" int cwipc_hip_tiles_used(cwipc_pointcloud *pc, uint8_t *used256) {
    if (pc == nullptr || used256 == nullptr) return -1;
    memset(used256, 0, 256);
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_tiles_used", pc, keep);
    if (!src) return -1;
    if (src->npoints == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    uint32_t *dev = (uint32_t *)c.dev_words;
    bool ok = hipMemsetAsync(dev, 0, 32, c.stream) == hipSuccess;
    if (ok) k::tiles_used(*src, dev, c.stream);
    ok = ok && hipMemcpyAsync(c.host_words, dev, 32, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    if (!ok) return -1;
    int count = 0;
    for (int t = 0; t < 256; t++) {
        used256[t] = (c.host_words[t >> 5] >> (t & 31)) & 1u;
        count += used256[t];
    }
    // a census: remembered on the cloud.  The cloud may be in other threads' hands (clouds are immutable but for this note): one
    // census at a time writes the words, and only a cloud that has no set yet gets one (a set a producer left is at least as good)
    {
        static std::mutex census_mutex;
        std::lock_guard<std::mutex> lock(census_mutex);
        if (!src->has_tiles.load(std::memory_order_acquire)) src->set_tiles(c.host_words);
    }
    return count;
}

// reference python/cwipc/filters/simulatecams.py:44-70 (hard = True): the per-point loop; the centroid is the caller's
extern "C" cwipc_pointcloud *cwipc_hip_simulatecams(cwipc_pointcloud *pc, int ncamera, float centroid_x, float centroid_z, const double *camera_dirs) {
    if (pc == nullptr || camera_dirs == nullptr || ncamera < 1 || ncamera > 32) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_simulatecams", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_rgbt(src);   // the coordinates do not change: the result holds the very same planes
    if (!dst) return nullptr;
    k::map_cameras(*src, *dst, ncamera, centroid_x, centroid_z, camera_dirs, c.stream);
    if (!c.sync()) return nullptr;
    inherit_first(*dst, *src);
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference python/cwipc/filters/simulatecams.py:60-69 (hard = False); the random stream is the library's (hip_ext.h), not numpy's
extern "C" cwipc_pointcloud *cwipc_hip_simulatecams_soft(cwipc_pointcloud *pc, int ncamera, float centroid_x, float centroid_z, const double *camera_dirs,
                                                         double skew, uint64_t seed) {
    if (pc == nullptr || camera_dirs == nullptr) return nullptr;
    if (ncamera < 2 || ncamera > 32) {
        // (the reference raises IndexError for one camera: there is no second one to draw against)
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_simulatecams_soft", "the soft rule needs between 2 and 32 cameras");
        return nullptr;
    }
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_simulatecams_soft", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_rgbt(src);   // the coordinates do not change: the result holds the very same planes
    if (!dst) return nullptr;
    k::map_cameras_soft(*src, *dst, ncamera, centroid_x, centroid_z, camera_dirs, skew, seed, c.stream);
    if (!c.sync()) return nullptr;
    inherit_first(*dst, *src);
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference python/cwipc/filters/noise.py:31-50; the random stream is the library's (hip_ext.h), not numpy's
extern "C" cwipc_pointcloud *cwipc_hip_noise(cwipc_pointcloud *pc, double distance, uint64_t seed) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_noise", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_xyz(src);   // colours and tiles do not change: the result holds the very same words
    if (!dst) return nullptr;
    k::map_noise(*src, *dst, distance, seed, c.stream);
    if (!c.sync()) return nullptr;
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference python/cwipc/filters/colorize.py:100-119
extern "C" cwipc_pointcloud *cwipc_hip_colorize(cwipc_pointcloud *pc, double weight, const double *lut, const uint8_t *valid) {
    if (pc == nullptr || lut == nullptr || valid == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_colorize", pc, keep);
    if (!src) return nullptr;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_with_new_rgbt(src);   // the coordinates do not change: the result holds the very same planes
    if (!dst) return nullptr;
    const int ndoubles = 1025 + 256;
    // (r4) A stream of frames colours every tile with the same weight and map: the table of a (device, weight, map) stays on the
    // device -- up to sixteen of them for the life of the process -- and a call that finds its table there is one kernel launch that
    // nobody waits for (the result carries an event, the input remembers its reader).  Round 3's call built the table, copied it
    // and waited for the kernel: 35 us per camera tile in config 5's chain, most of it the wait.
    struct CachedTable { int device; double weight; double lut[768]; uint8_t valid[256]; double *dev; };
    static std::mutex cache_mutex;
    static std::vector<CachedTable *> cache;
    double *dev_table = nullptr;
    {
        std::lock_guard<std::mutex> lock(cache_mutex);
        for (CachedTable *t : cache)
            if (t->device == src->device && memcmp(&t->weight, &weight, sizeof(double)) == 0 && memcmp(t->lut, lut, sizeof(t->lut)) == 0 &&
                memcmp(t->valid, valid, sizeof(t->valid)) == 0) { dev_table = t->dev; break; }
    }
    if (dev_table && !profiling_enabled()) {
        // (on the thread's second stream: cwipc_downsample takes "the thread's first stream is busy" for calls that come faster than
        // its workspace turns around and answers with another workspace, 0.3 GB of leaf grids -- a kernel of this filter in flight
        // there made every thread of config 5's chain hold three, test_config5_eight_threads_workspace_footprint)
        hipStream_t s = c.stream_alt ? c.stream_alt : c.stream;
        if (s != c.stream) src->wait_on(s);   // (device_input has ordered the first stream behind the input's producer, not this one)
        k::map_colorize(*src, *dst, dev_table, s);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) {
            hip_failed(e, "cwipc_hip_colorize", __FILE__, __LINE__);
            (void)c.sync();
            return nullptr;
        }
        dst->mark_pending(s);
        src->note_reader(s);
        inherit_first(*dst, *src);
        dst->set_tiles_from(*src);   // (colours change, tiles do not)
        return wrap(dst, pc->timestamp(), pc->cellsize());
    }
    const bool cached = dev_table != nullptr;
    double *host_table = (double *)c.staging(ndoubles * sizeof(double));
    if (!host_table) return nullptr;
    // the same IEEE double operations Python performs, in the same order
    for (int t = 0; t < 256; t++)
        for (int ch = 0; ch < 3; ch++) host_table[t * 3 + ch] = lut[t * 3 + ch] * weight;
    for (int v = 0; v < 256; v++) host_table[768 + v] = v / 255.0;
    host_table[1024] = 1 - weight;
    for (int t = 0; t < 256; t++) host_table[1025 + t] = valid[t] ? 1.0 : 0.0;
    bool ok = true;
    if (!cached) {
        dev_table = (double *)pool_alloc(ndoubles * sizeof(double));
        if (!dev_table) return nullptr;
        ok = hipMemcpyAsync(dev_table, host_table, ndoubles * sizeof(double), hipMemcpyHostToDevice, c.stream) == hipSuccess;
    }
    if (ok) k::map_colorize(*src, *dst, dev_table, c.stream);
    ok = c.sync() && ok;
    if (!cached) {
        bool kept = false;
        if (ok) {
            std::lock_guard<std::mutex> lock(cache_mutex);
            if (cache.size() < 16) {
                auto *t = new CachedTable();
                t->device = src->device; t->weight = weight; t->dev = dev_table;
                memcpy(t->lut, lut, sizeof(t->lut)); memcpy(t->valid, valid, sizeof(t->valid));
                cache.push_back(t);   // (the block stays out of the pool from here on)
                kept = true;
            }
        }
        if (!kept) pool_free(dev_table);
    }
    if (!ok) return nullptr;
    inherit_first(*dst, *src);
    dst->set_tiles_from(*src);   // (colours change, tiles do not)
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

// reference src/cwipc_filters.cpp:388-418; n-ary form = left fold (python/cwipc/util.py:1330-1332)
extern "C" cwipc_pointcloud *cwipc_hip_join_multi(cwipc_pointcloud **pcs, int npc) {
    if (pcs == nullptr || npc <= 0) return nullptr;
    for (int i = 0; i < npc; i++) if (pcs[i] == nullptr) return nullptr;
    std::vector<std::unique_ptr<cwipc_hip_pointcloud>> keep(npc);
    std::vector<std::shared_ptr<DeviceSoA>> src(npc);
    size_t total = 0;
    for (int i = 0; i < npc; i++) {
        src[i] = device_input("cwipc_join", pcs[i], keep[i]);
        if (!src[i]) {
            cwipc_log(CWIPC_LOG_LEVEL_WARNING, "cwipc_join", "some pcl_pointcloud is NULL");
            return nullptr;
        }
        total += src[i]->npoints;
    }
    uint64_t ts = pcs[0]->timestamp();
    float cellsize = pcs[0]->cellsize();
    for (int i = 1; i < npc; i++) {
        ts = std::min(ts, pcs[i]->timestamp());
        cellsize = std::min(cellsize, pcs[i]->cellsize());
    }
    // all points in one of the inputs (the others are empty): the result holds that input's planes, nothing is copied
    for (int i = 0; i < npc; i++) {
        if (src[i]->npoints == total && total > 0) return wrap(src[i], ts, cellsize);
    }
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    auto dst = soa_alloc(total);
    if (!dst) return nullptr;
    size_t off = 0;
    for (int i = 0; i < npc; i++) {
        k::JoinPart part{src[i]->x(), src[i]->y(), src[i]->z(), src[i]->rgbt(), src[i]->npoints, off};
        k::join_copy(part, *dst, c.stream);
        off += src[i]->npoints;
    }
    if (profiling_enabled()) {
        if (!c.sync()) return nullptr;
        return wrap(dst, ts, cellsize);
    }
    // the copies need no more attention from the host: the result goes out with them still running (it carries an event),
    // the inputs stay until they have been read
    if (hipError_t e = hipGetLastError(); e != hipSuccess) {
        hip_failed(e, "cwipc_join", __FILE__, __LINE__);
        (void)c.sync();
        return nullptr;
    }
    dst->mark_pending(c.stream);
    for (int i = 0; i < npc; i++) if (src[i]->npoints) src[i]->note_reader(c.stream);
    {   // the tiles that may occur: the union over the parts that hold points (unknown as soon as one of them is)
        bool known = true;
        uint32_t u[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < npc; i++) {
            if (!src[i]->npoints) continue;
            known = known && src[i]->has_tiles;
            for (int w = 0; w < 8; w++) u[w] |= src[i]->tiles[w];
        }
        if (known) dst->set_tiles(u);
    }
    return wrap(dst, ts, cellsize);
}

extern "C" cwipc_pointcloud *cwipc_join(cwipc_pointcloud *pc1, cwipc_pointcloud *pc2) {
    if (pc1 == nullptr || pc2 == nullptr) return nullptr;
    cwipc_pointcloud *both[2] = {pc1, pc2};
    return cwipc_hip_join_multi(both, 2);
}

// ---------------------------------------------------------------------------
// reference src/cwipc_filters.cpp:30-172
// ---------------------------------------------------------------------------
extern "C" cwipc_pointcloud *cwipc_downsample(cwipc_pointcloud *pc, float cellsize) {
    bool leaf_split = true;
    const char *who = "cwipc_downsample";
    if (cellsize < 0) {          // :90-92 -> cwipc_downsample_voxelgrid(pc, -cellsize)
        cellsize = -cellsize;
        leaf_split = false;
        who = "cwipc_downsample_voxelgrid";
    }
    if (pc == nullptr) return nullptr;
    if (cwipc_hip_device_count() > current_device()) voxel_sample_streams();   // (before the input puts a wait into this thread's stream)
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input(who, pc, keep);
    if (!src) return nullptr;
    float oldcellsize = pc->cellsize();   // :42-46, :103-107
    if (oldcellsize >= cellsize) cellsize = oldcellsize;
    if (src->npoints == 0) {
        if (leaf_split) return wrap(soa_alloc(0), pc->timestamp(), cellsize);   // zero leaves -> empty cloud
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_downsample", "VoxelGrid filter produced empty pointcloud");   // :58-62
        return nullptr;
    }
    int err = 0;
    std::shared_ptr<DeferredResult> pending;
    auto dst = voxel_downsample(src, cellsize, leaf_split, &err, &pending);
    if (pending) {
        // a stream of frames: the result is handed out while its kernels run (it settles when somebody asks for its points)
        auto *rv = new cwipc_hip_pointcloud();
        rv->adopt_deferred(pending, pc->timestamp(), cellsize);
        return rv;
    }
    if (!dst) return nullptr;
    return wrap(dst, pc->timestamp(), cellsize);
}

// ---------------------------------------------------------------------------
// reference src/cwipc_filters.cpp:181-278
// ---------------------------------------------------------------------------
namespace {

// The inner overload (:181-211): SOR over one cloud's planes.
std::shared_ptr<DeviceSoA> sor_once(const DeviceSoA &src, int k, float stddev_mul) {
    if (src.npoints == 0) return soa_alloc(0);
    // d_i, then the threshold (on the device: nothing is read back in between), then the compaction, whose
    // wait is the only one after the k-NN grid has been set up
    float *dist = (float *)pool_alloc(src.npoints * sizeof(float) + 256);
    if (!dist) return nullptr;
    double *thr_dev = reinterpret_cast<double *>(reinterpret_cast<char *>(dist) + ((src.npoints * sizeof(float) + 127) & ~(size_t)127));
    std::shared_ptr<DeviceSoA> out;
    if (sor_mean_distances(src, k, dist)) out = sor_threshold_and_select(src, dist, stddev_mul, thr_dev);
    // every failure exit: kernels that read or write `dist` may still be in flight, and the block goes back to a pool
    // other threads allocate from
    if (!out) (void)tctx().sync();
    pool_free(dist);
    return out;
}

}  // namespace

extern "C" cwipc_pointcloud *cwipc_remove_outliers(cwipc_pointcloud *pc, int kNeighbors, float stddevMulThresh, bool perTile) {
    if (pc == nullptr) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_remove_outliers", pc, keep);
    if (!src) return nullptr;
    if (!perTile) {   // :262-268
        return wrap(sor_once(*src, kNeighbors, stddevMulThresh), pc->timestamp(), pc->cellsize());
    }
    // :238-261 -- distinct tiles in first-appearance order: a kernel leaves the index of every tile value's first point
    // in 256 words, the host sorts the tiles that occur by it (1 KB read back, the tile plane stays where it is).
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    size_t n = src->npoints;
    std::vector<int> tiles;
    if (n) {
        uint32_t *dev_first = (uint32_t *)c.device_scratch(256 * sizeof(uint32_t));
        uint32_t *first = (uint32_t *)c.staging(256 * sizeof(uint32_t));
        if (!dev_first || !first) return nullptr;
        k::tile_first_index(*src, dev_first, c.stream);
        bool ok = hipMemcpyAsync(first, dev_first, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = c.sync() && ok;
        if (!ok) return nullptr;
        std::vector<std::pair<uint32_t, int>> order;
        for (int t = 0; t < 256; t++) if (first[t] != 0xffffffffu) order.emplace_back(first[t], t);
        std::sort(order.begin(), order.end());
        for (auto &o : order) tiles.push_back(o.second);
    }
    std::vector<std::shared_ptr<DeviceSoA>> parts;
    size_t total = 0;
    for (int tile : tiles) {
        k::Predicate p{};
        p.mode = 0;          // cwipc_tilefilter semantics, including tile 0 = wildcard (:252, :296)
        p.tile = tile;
        auto sub = compact(*src, p);
        if (!sub) return nullptr;
        auto cleaned = sor_once(*sub, kNeighbors, stddevMulThresh);
        if (!cleaned) return nullptr;
        total += cleaned->npoints;
        parts.push_back(cleaned);
    }
    auto dst = soa_alloc(total);
    if (!dst) return nullptr;
    size_t off = 0;
    for (auto &part : parts) {
        k::JoinPart jp{part->x(), part->y(), part->z(), part->rgbt(), part->npoints, off};
        k::join_copy(jp, *dst, c.stream);
        off += part->npoints;
    }
    if (!c.sync()) return nullptr;
    return wrap(dst, pc->timestamp(), pc->cellsize());
}

extern "C" int cwipc_hip_knn_mean_dist(cwipc_pointcloud *pc, int kNeighbors, float *mean_dist, size_t cap, double *threshold, float stddevMulThresh) {
    if (pc == nullptr) return -1;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_knn_mean_dist", pc, keep);
    if (!src) return -1;
    size_t n = src->npoints;
    if (cap < n) return -1;
    if (n == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    float *dist = (float *)pool_alloc(n * sizeof(float));
    if (!dist) return -1;
    bool ok = sor_mean_distances(*src, kNeighbors, dist);
    double thr = 0;
    if (ok && threshold) ok = sor_threshold(dist, n, stddevMulThresh, &thr);
    if (ok) {
        void *stage = c.staging(n * sizeof(float));
        ok = stage && hipMemcpyAsync(stage, dist, n * sizeof(float), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = c.sync() && ok;
        if (ok) memcpy(mean_dist, stage, n * sizeof(float));
    }
    pool_free(dist);
    if (ok && threshold) *threshold = thr;
    return ok ? 0 : -1;
}

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/util.py:114-143 (cwipc_direction_filter)
// ---------------------------------------------------------------------------
namespace {

bool direction_args_ok(const char *who, float radius, int max_nn) {
    if (radius > 0.f && std::isfinite(radius) && max_nn >= 1 && max_nn <= DIRECTION_MAX_NN) return true;
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "radius must be positive and finite, max_nn between 1 and 128");
    return false;
}

}  // namespace

extern "C" cwipc_pointcloud *cwipc_hip_direction_filter(cwipc_pointcloud *pc, double dx, double dy, double dz, double threshold, float radius, int max_nn) {
    if (pc == nullptr) return nullptr;
    if (!direction_args_ok("cwipc_hip_direction_filter", radius, max_nn)) return nullptr;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_direction_filter", pc, keep);
    if (!src) return nullptr;
    const size_t n = src->npoints;
    if (n == 0) return wrap(soa_alloc(0), pc->timestamp(), pc->cellsize());
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    // the reference divides by the norm unless it is 0 (a zero direction: every dot product is 0)
    double dir[3] = {dx, dy, dz};
    const double len = sqrt(dx * dx + dy * dy + dz * dz);
    if (len != 0.0) for (double &v : dir) v /= len;
    // the decision as a float plane (0 keep, 1 drop) and the outlier filter's compaction (mode 3: keep iff !(plane > 0.5))
    float *drop = (float *)pool_alloc(n * sizeof(float) + 256);
    if (!drop) return nullptr;
    double *cen = reinterpret_cast<double *>(reinterpret_cast<char *>(drop) + ((n * sizeof(float) + 127) & ~(size_t)127));
    std::shared_ptr<DeviceSoA> out;
    if (direction_normals(*src, radius, max_nn, dir, threshold, drop, nullptr, 0, nullptr, cen)) out = sor_select(*src, drop, 0.5);
    if (!out) (void)c.sync();   // kernels that write `drop` may still be in flight
    pool_free(drop);
    return wrap(out, pc->timestamp(), pc->cellsize());
}

extern "C" int cwipc_hip_estimate_normals(cwipc_pointcloud *pc, float radius, int max_nn, float *normals, uint32_t *nn_count, float *centroid, size_t cap) {
    if (pc == nullptr || (normals == nullptr && nn_count != nullptr)) return -1;
    if (!direction_args_ok("cwipc_hip_estimate_normals", radius, max_nn)) return -1;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = device_input("cwipc_hip_estimate_normals", pc, keep);
    if (!src) return -1;
    const size_t n = src->npoints;
    if (normals && cap < n) return -1;
    if (n == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    // one block: normals (3 x n floats) | counts (n words) | centroid (3 doubles)
    const size_t nb = 3 * n * sizeof(float), cb = n * sizeof(uint32_t);
    const size_t cen_at = (nb + cb + 127) & ~(size_t)127, bytes = cen_at + 3 * sizeof(double);
    char *block = (char *)pool_alloc(bytes);
    if (!block) return -1;
    float *dn = (float *)block;
    uint32_t *dc = (uint32_t *)(block + nb);
    double *dcen = (double *)(block + cen_at);
    const double zero[3] = {0, 0, 0};
    bool ok = direction_normals(*src, radius, max_nn, zero, 0.0, nullptr, normals ? dn : nullptr, n, normals ? dc : nullptr, dcen);
    if (ok) {
        char *stage = (char *)c.staging(bytes);
        ok = stage && hipMemcpyAsync(stage, block, bytes, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = c.sync() && ok;
        if (ok) {
            // the caller's normals are three planes of `cap` floats
            if (normals) for (int a = 0; a < 3; a++) memcpy(normals + (size_t)a * cap, stage + (size_t)a * n * sizeof(float), n * sizeof(float));
            if (nn_count) memcpy(nn_count, stage + nb, cb);
            if (centroid) {
                const double *hc = (const double *)(stage + cen_at);
                for (int a = 0; a < 3; a++) centroid[a] = (float)hc[a];
            }
        }
    } else {
        (void)c.sync();
    }
    pool_free(block);
    return ok ? 0 : -1;
}

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/analyze.py:116-123 (the KD-tree query) and :171-179 (gaussian_kde)
// ---------------------------------------------------------------------------
extern "C" int cwipc_hip_nn_distance2(cwipc_pointcloud *source, cwipc_pointcloud *reference, int nth, double max_distance, double *dist2, size_t cap) {
    const char *who = "cwipc_hip_nn_distance2";
    if (source == nullptr || reference == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return -1;
    }
    if (nth < 0 || nth > NN_MAX_NTH || !(max_distance > 0.0)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "nth must lie between 0 and 31, max_distance must be positive (inf: no bound)");
        return -1;
    }
    std::unique_ptr<cwipc_hip_pointcloud> keep_src, keep_ref;
    auto src = device_input(who, source, keep_src);
    if (!src) return -1;
    auto ref = source == reference ? src : device_input(who, reference, keep_ref);
    if (!ref) return -1;
    const size_t n = src->npoints;
    if (cap < n || (n && dist2 == nullptr)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the result array is too small");
        return -1;
    }
    if (n == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    double *dev = (double *)pool_alloc(n * sizeof(double));
    if (!dev) return -1;
    bool ok = nn_distance2(*src, *ref, nth, max_distance, dev);
    ok = ok && hipMemcpyAsync(dist2, dev, n * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;   // (also on failure: kernels that write `dev` may still be in flight)
    pool_free(dev);
    return ok ? 0 : -1;
}

extern "C" int cwipc_hip_nn_distance2_jobs(cwipc_pointcloud *source, cwipc_pointcloud *reference, const cwipc_hip_nn_job *jobs, int njobs, double *dist2,
                                           size_t cap) {
    const char *who = "cwipc_hip_nn_distance2_jobs";
    if (source == nullptr || reference == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return -1;
    }
    if (jobs == nullptr || njobs < 1 || njobs > NN_MAX_JOBS) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "between 1 and 64 jobs");
        return -1;
    }
    for (int j = 0; j < njobs; j++) {
        const cwipc_hip_nn_job &b = jobs[j];
        if (b.nth < 0 || b.nth > NN_MAX_NTH || !(b.max_distance > 0.0) || std::isnan(b.source_y[0]) || std::isnan(b.source_y[1]) ||
            std::isnan(b.reference_y[0]) || std::isnan(b.reference_y[1])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "nth must lie between 0 and 31, max_distance must be positive (inf: no bound), a y limit is not NaN");
            return -1;
        }
    }
    std::unique_ptr<cwipc_hip_pointcloud> keep_src, keep_ref;
    auto src = device_input(who, source, keep_src);
    if (!src) return -1;
    auto ref = source == reference ? src : device_input(who, reference, keep_ref);
    if (!ref) return -1;
    const size_t n = src->npoints;
    if (cap < n || (n && dist2 == nullptr)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the result array is too small");
        return -1;
    }
    if (n == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    double *dev = (double *)pool_alloc((size_t)njobs * n * sizeof(double));
    void *table = pool_alloc(nn_jobs_table_bytes(njobs));
    if (!dev || !table) { pool_free(dev); pool_free(table); return -1; }
    bool ok = nn_distance2_jobs(*src, *ref, jobs, njobs, dev, table);
    if (ok && cap == n) {
        ok = hipMemcpyAsync(dist2, dev, (size_t)njobs * n * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    } else {
        for (int j = 0; ok && j < njobs; j++)
            ok = hipMemcpyAsync(dist2 + (size_t)j * cap, dev + (size_t)j * n, n * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    }
    ok = c.sync() && ok;   // (also on failure: kernels that read the table and write `dev` may still be in flight)
    pool_free(dev);
    pool_free(table);
    return ok ? 0 : -1;
}

extern "C" int cwipc_hip_gaussian_kde(const double *samples, size_t n, double h, const double *at, size_t m, double *density) {
    const char *who = "cwipc_hip_gaussian_kde";
    if (n == 0 || samples == nullptr || !(h > 0.0) || !std::isfinite(h) || (m && (at == nullptr || density == nullptr))) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "needs at least one sample, a positive, finite bandwidth and arrays for the evaluation points");
        return -1;
    }
    if (m == 0) return 0;
    if (!device_available(who)) return -1;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    // one block: samples | evaluation points | densities
    double *block = (double *)pool_alloc((n + 2 * m) * sizeof(double));
    if (!block) return -1;
    double *ds = block, *da = block + n, *dd = block + n + m;
    bool ok = hipMemcpyAsync(ds, samples, n * sizeof(double), hipMemcpyHostToDevice, c.stream) == hipSuccess &&
              hipMemcpyAsync(da, at, m * sizeof(double), hipMemcpyHostToDevice, c.stream) == hipSuccess;
    ok = ok && gaussian_kde(ds, n, h, da, m, dd);
    ok = ok && hipMemcpyAsync(density, dd, m * sizeof(double), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(block);
    return ok ? 0 : -1;
}

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/fine.py (open3d registration_icp) and analyze.py's OverlapAnalyzer (evaluate_registration):
// kernels_icp.hip
// ---------------------------------------------------------------------------
namespace {

const double ICP_IDENTITY[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// The scalar arguments of the ICP entry points are checked HERE, once (kernels_icp.hip takes them as checked), in the order of the
// helpers below; false: logged.
struct IcpClouds {
    std::unique_ptr<cwipc_hip_pointcloud> keep_src, keep_ref;
    std::shared_ptr<DeviceSoA> src, ref;
};

// both clouds on the device, and the arguments every ICP entry point has
bool icp_inputs(const char *who, cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance, IcpClouds &in) {
    if (source == nullptr || reference == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return false;
    }
    if (!(max_distance > 0.0)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_distance must be positive (inf: no bound)");
        return false;
    }
    for (int i = 0; T && i < 16; i++)
        if (!std::isfinite(T[i])) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the matrix must be finite");
            return false;
        }
    in.src = device_input(who, source, in.keep_src);
    if (!in.src) return false;
    in.ref = source == reference ? in.src : device_input(who, reference, in.keep_ref);
    return (bool)in.ref;
}

bool icp_criteria_ok(const char *who, const IcpCriteria &k) {
    if (k.max_iteration >= 0 && !std::isnan(k.relative_fitness) && !std::isnan(k.relative_rmse)) return true;
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "max_iteration must not be negative, the criteria not NaN");
    return false;
}

bool gicp_epsilon_ok(const char *who, double epsilon) {
    if (epsilon > 0.0 && std::isfinite(epsilon)) return true;
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "epsilon must be positive and finite");
    return false;
}

// an entry point's body between the C caller and C++: 0 / -1, no exception leaves
template <class Body>
int icp_entry(const char *who, Body &&body) {
    try {
        return body() ? 0 : -1;
    } catch (...) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "exception");
        return -1;
    }
}

// What an aligner starts from, which is also what its caller gets when it fails; and a result into the caller's optional pointers.
IcpResult icp_start(const double *init) {
    IcpResult r{};
    memcpy(r.T, init ? init : ICP_IDENTITY, sizeof(r.T));
    return r;
}

void icp_result_out(const IcpResult &r, double *T_out, double *fitness, double *inlier_rmse, int *iterations) {
    if (T_out) memcpy(T_out, r.T, sizeof(r.T));
    if (fitness) *fitness = r.fitness;
    if (inlier_rmse) *inlier_rmse = r.inlier_rmse;
    if (iterations) *iterations = r.iterations;
}

void icp_sums_out(uint64_t hn, const double *hs, int count, uint64_t *n, double *sums) {
    if (n) *n = hn;
    if (sums) memcpy(sums, hs, (size_t)count * sizeof(double));
}

}  // namespace

extern "C" int cwipc_hip_correspondences(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance, uint32_t *idx,
                                         double *dist2, size_t cap) {
    const char *who = "cwipc_hip_correspondences";
    return icp_entry(who, [&] {
        IcpClouds in;
        if (!icp_inputs(who, source, reference, T, max_distance, in)) return false;
        const size_t n = in.src->npoints;
        if (cap < n) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the result arrays are too small");
            return false;
        }
        return n == 0 || icp_correspondences(*in.src, *in.ref, T ? T : ICP_IDENTITY, max_distance, idx, dist2);
    });
}

extern "C" int cwipc_hip_icp_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance, const double *cp,
                                  const double *cq, uint64_t *n, double *sums) {
    const char *who = "cwipc_hip_icp_sums";
    uint64_t hn = 0;
    double hs[16] = {};
    icp_sums_out(hn, hs, 16, n, sums);
    return icp_entry(who, [&] {
        IcpClouds in;
        if (!icp_inputs(who, source, reference, T, max_distance, in)) return false;
        const double zero[3] = {0, 0, 0};
        if (!icp_sums(*in.src, *in.ref, T ? T : ICP_IDENTITY, max_distance, cp ? cp : zero, cq ? cq : zero, &hn, hs)) return false;
        icp_sums_out(hn, hs, 16, n, sums);
        return true;
    });
}

extern "C" int cwipc_hip_icp_point2point(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init,
                                         double relative_fitness, double relative_rmse, int max_iteration, double *T_out, double *fitness,
                                         double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_point2point";
    IcpResult res = icp_start(init);
    icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
    return icp_entry(who, [&] {
        IcpClouds in;
        const IcpCriteria k{relative_fitness, relative_rmse, max_iteration};
        if (!icp_inputs(who, source, reference, init, max_distance, in) || !icp_criteria_ok(who, k)) return false;
        if (in.src->npoints == 0 || in.ref->npoints == 0) return true;
        // the pivots, once per run: the clouds' centroids ((0, 0, 0) for a cloud with a non-finite point: any pivot is right,
        // a near one only keeps the covariance from cancelling)
        double cp0[3], cq[3];
        if (!icp_centroid(*in.src, cp0) || !icp_centroid(*in.ref, cq)) return false;
        if (!(std::isfinite(cp0[0]) && std::isfinite(cp0[1]) && std::isfinite(cp0[2]))) cp0[0] = cp0[1] = cp0[2] = 0.0;
        if (!(std::isfinite(cq[0]) && std::isfinite(cq[1]) && std::isfinite(cq[2]))) cq[0] = cq[1] = cq[2] = 0.0;
        if (!icp_point2point(*in.src, *in.ref, max_distance, k, cp0, cq, res)) return false;
        icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
        return true;
    });
}

extern "C" int cwipc_hip_icp_plane_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance, const float *normals,
                                        float radius, int max_nn, uint64_t *n, double *sums) {
    const char *who = "cwipc_hip_icp_plane_sums";
    uint64_t hn = 0;
    double hs[29] = {};
    icp_sums_out(hn, hs, 29, n, sums);
    return icp_entry(who, [&] {
        IcpClouds in;
        if (!icp_inputs(who, source, reference, T, max_distance, in)) return false;
        if (!normals && !direction_args_ok(who, radius, max_nn)) return false;
        if (!icp_plane_sums(*in.src, *in.ref, T ? T : ICP_IDENTITY, max_distance, normals, radius, max_nn, &hn, hs)) return false;
        icp_sums_out(hn, hs, 29, n, sums);
        return true;
    });
}

extern "C" int cwipc_hip_icp_point2plane(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init, const float *normals,
                                         float radius, int max_nn, double relative_fitness, double relative_rmse, int max_iteration, double *T_out,
                                         double *fitness, double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_point2plane";
    IcpResult res = icp_start(init);
    icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
    return icp_entry(who, [&] {
        IcpClouds in;
        const IcpCriteria k{relative_fitness, relative_rmse, max_iteration};
        if (!icp_inputs(who, source, reference, init, max_distance, in)) return false;
        if (!normals && !direction_args_ok(who, radius, max_nn)) return false;
        if (!icp_criteria_ok(who, k)) return false;
        if (!icp_point2plane(*in.src, *in.ref, max_distance, normals, radius, max_nn, k, res)) return false;
        icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
        return true;
    });
}

extern "C" int cwipc_hip_gicp_covariances(cwipc_pointcloud *pc, const float *normals, float radius, int max_nn, const double *direction, double epsilon,
                                          double *cov, size_t cap) {
    const char *who = "cwipc_hip_gicp_covariances";
    return icp_entry(who, [&] {
        if (pc == nullptr) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
            return false;
        }
        if (!gicp_epsilon_ok(who, epsilon)) return false;
        if (!normals && !direction_args_ok(who, radius, max_nn)) return false;
        std::unique_ptr<cwipc_hip_pointcloud> keep;
        auto src = device_input(who, pc, keep);
        if (!src) return false;
        const size_t n = src->npoints;
        if (cap < n || (n && cov == nullptr)) {
            cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "the result array is too small");
            return false;
        }
        return icp_gicp_covariances(*src, normals, radius, max_nn, direction, epsilon, cov);
    });
}

extern "C" int cwipc_hip_icp_gicp_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance,
                                       const float *source_normals, const float *reference_normals, float radius, int max_nn, double epsilon, uint64_t *n,
                                       double *sums) {
    const char *who = "cwipc_hip_icp_gicp_sums";
    uint64_t hn = 0;
    double hs[29] = {};
    icp_sums_out(hn, hs, 29, n, sums);
    return icp_entry(who, [&] {
        IcpClouds in;
        if (!icp_inputs(who, source, reference, T, max_distance, in)) return false;
        if (!(source_normals && reference_normals) && !direction_args_ok(who, radius, max_nn)) return false;
        if (!gicp_epsilon_ok(who, epsilon)) return false;
        if (!icp_gicp_sums(*in.src, *in.ref, T ? T : ICP_IDENTITY, max_distance, source_normals, reference_normals, radius, max_nn, epsilon, &hn, hs)) return false;
        icp_sums_out(hn, hs, 29, n, sums);
        return true;
    });
}

extern "C" int cwipc_hip_icp_generalized(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init,
                                         const float *source_normals, const float *reference_normals, float radius, int max_nn, double epsilon,
                                         double relative_fitness, double relative_rmse, int max_iteration, double *T_out, double *fitness,
                                         double *inlier_rmse, int *iterations) {
    const char *who = "cwipc_hip_icp_generalized";
    IcpResult res = icp_start(init);
    icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
    return icp_entry(who, [&] {
        IcpClouds in;
        const IcpCriteria k{relative_fitness, relative_rmse, max_iteration};
        if (!icp_inputs(who, source, reference, init, max_distance, in)) return false;
        if (!(source_normals && reference_normals) && !direction_args_ok(who, radius, max_nn)) return false;
        if (!gicp_epsilon_ok(who, epsilon) || !icp_criteria_ok(who, k)) return false;
        if (!icp_generalized(*in.src, *in.ref, max_distance, source_normals, reference_normals, radius, max_nn, epsilon, k, res)) return false;
        icp_result_out(res, T_out, fitness, inlier_rmse, iterations);
        return true;
    });
}

// ---------------------------------------------------------------------------
// reference python/cwipc/registration/util.py:146-229: the floor and tile helpers (kernels_floor.hip)
// ---------------------------------------------------------------------------
namespace {

// count -> scan -> (wait: the two totals size the result) -> scatter -> wait
std::shared_ptr<DeviceSoA> floor_partition(const std::shared_ptr<DeviceSoA> &src, const k::FloorArgs &a, uint64_t *n_first) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    if (n_first) *n_first = 0;
    const size_t n = src->npoints;
    if (n == 0) return soa_alloc(0);
    const size_t nb = k::floor_blocks(n);
    uint32_t *counts = (uint32_t *)c.device_scratch((2 * nb + 2) * sizeof(uint32_t));
    if (!counts) return nullptr;
    const uint32_t tag = ++c.tag ? c.tag : ++c.tag;
    volatile unsigned long long *words = reinterpret_cast<volatile unsigned long long *>(c.host_words);
    words[0] = words[1] = 0ull;
    k::floor_count(*src, a, counts, c.stream);
    k::floor_scan(counts, nb, reinterpret_cast<unsigned long long *>(c.host_words), tag, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = c.sync() && ok;
    if (!ok || (uint32_t)(words[0] >> 32) != tag || (uint32_t)(words[1] >> 32) != tag) {
        hip_failed(hipGetLastError(), "floor partition", __FILE__, __LINE__);
        return nullptr;
    }
    const size_t na = (uint32_t)words[0], nrest = (uint32_t)words[1];
    if (na + nrest > n) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip", "floor partition: inconsistent count");
        return nullptr;
    }
    if (n_first) *n_first = na;
    if (na == n || nrest == n) {
        // one class holds every point: the result is the input, point for point -- it holds the input's planes (clouds are immutable)
        auto same = std::make_shared<DeviceSoA>();
        same->xyz_block = src->xyz_block;
        same->rgbt_block = src->rgbt_block;
        same->npoints = src->npoints;
        same->stride = src->stride;
        same->device = src->device;
        same->set_tiles_from(*src);
        return same;
    }
    auto dst = soa_alloc(na + nrest);
    if (!dst) return nullptr;
    if (na + nrest) {
        k::floor_scatter(*src, a, counts, *dst, c.stream);
        ok = hipGetLastError() == hipSuccess;
        ok = c.sync() && ok;
        if (!ok) { hip_failed(hipGetLastError(), "floor partition", __FILE__, __LINE__); return nullptr; }
    }
    dst->set_tiles_from(*src);   // (a subset of the points: what could not occur still cannot)
    return dst;
}

std::shared_ptr<DeviceSoA> floor_input(const char *who, cwipc_pointcloud *pc, std::unique_ptr<cwipc_hip_pointcloud> &keep) {
    if (pc == nullptr) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, who, "NULL pointcloud");
        return nullptr;
    }
    return device_input(who, pc, keep);
}

}  // namespace

extern "C" cwipc_pointcloud *cwipc_hip_floor_partition(cwipc_pointcloud *pc, double level, int flags, double radius, uint64_t *n_first) {
    if (n_first) *n_first = 0;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_floor_partition", pc, keep);
    if (!src) return nullptr;
    // (cellsize 0: the reference builds its result with cwipc_from_numpy_matrix and does not copy the cellsize, util.py:154, :228)
    return wrap(floor_partition(src, k::FloorArgs{level, radius, flags}, n_first), pc->timestamp(), 0.f);
}

extern "C" cwipc_pointcloud *cwipc_hip_randomize_floor(cwipc_pointcloud *pc, double level, uint64_t seed) {
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_randomize_floor", pc, keep);
    if (!src) return nullptr;
    uint64_t n_first = 0;
    auto parted = floor_partition(src, k::FloorArgs{level, 0.0, k::FLOOR_KEEP_FLOOR | k::FLOOR_KEEP_REST}, &n_first);
    if (!parted) return nullptr;
    if (n_first < 2) return wrap(parted, pc->timestamp(), 0.f);   // nothing to permute
    ThreadCtx &c = tctx();
    auto dst = soa_with_new_rgbt(parted);   // the coordinates do not change: the result holds the very same planes
    if (!dst) return nullptr;
    bool ok = k::floor_shuffle(parted->rgbt(), (size_t)n_first, parted->npoints, seed, dst->rgbt(), c.stream);
    ok = ok && hipGetLastError() == hipSuccess;
    ok = c.sync() && ok;
    if (!ok) return nullptr;
    dst->set_tiles_from(*parted);   // (the same tile bytes in another order)
    return wrap(dst, pc->timestamp(), 0.f);
}

extern "C" int cwipc_hip_floor_radius_stats(cwipc_pointcloud *pc, double level, uint64_t count[2], float stat[4]) {
    if (count) count[0] = count[1] = 0;
    if (stat) for (int i = 0; i < 4; i++) stat[i] = NAN;
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_floor_radius_stats", pc, keep);
    if (!src || count == nullptr || stat == nullptr) return -1;
    if (src->npoints == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    uint32_t *state = (uint32_t *)pool_alloc(k::floor_radius_state_bytes());
    if (!state) return -1;
    k::floor_radius_select(*src, level, state, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(c.host_words, state, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;   // (also on failure: kernels that write `state` may still be in flight)
    pool_free(state);
    if (!ok) return -1;
    count[0] = c.host_words[0];
    count[1] = c.host_words[1];
    memcpy(stat, c.host_words + 2, 4 * sizeof(float));
    return 0;
}

extern "C" int cwipc_hip_tile_counts(cwipc_pointcloud *pc, int nonfloor_only, double level, uint64_t counts[256]) {
    if (counts) memset(counts, 0, 256 * sizeof(uint64_t));
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_tile_counts", pc, keep);
    if (!src || counts == nullptr) return -1;
    if (src->npoints == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    unsigned long long *dev = (unsigned long long *)pool_alloc(256 * sizeof(unsigned long long));
    void *stage = c.staging(256 * sizeof(unsigned long long));
    if (!dev || !stage) { pool_free(dev); return -1; }
    k::tile_histogram(*src, nonfloor_only ? 1 : 0, level, dev, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(stage, dev, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(dev);
    if (!ok) return -1;
    memcpy(counts, stage, 256 * sizeof(uint64_t));
    return 0;
}

extern "C" int cwipc_hip_bounds(cwipc_pointcloud *pc, float minmax[6]) {
    if (minmax) for (int a = 0; a < 3; a++) { minmax[a] = INFINITY; minmax[3 + a] = -INFINITY; }
    std::unique_ptr<cwipc_hip_pointcloud> keep;
    auto src = floor_input("cwipc_hip_bounds", pc, keep);
    if (!src || minmax == nullptr) return -1;
    if (src->npoints == 0) return 0;
    ThreadCtx &c = tctx();
    if (!c.ensure()) return -1;
    const unsigned nb = k::bounds_blocks(src->npoints);
    const size_t bytes = (size_t)nb * 6 * sizeof(float);
    float *partial = (float *)pool_alloc(bytes);
    float *host = (float *)c.staging(bytes);
    if (!partial || !host) { pool_free(partial); return -1; }
    k::bounds_partial(*src, partial, c.stream);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && hipMemcpyAsync(host, partial, bytes, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
    ok = c.sync() && ok;
    pool_free(partial);
    if (!ok) return -1;
    for (unsigned b = 0; b < nb; b++)
        for (int a = 0; a < 3; a++) {
            minmax[a] = fminf(minmax[a], host[b * 6 + a]);
            minmax[3 + a] = fmaxf(minmax[3 + a], host[b * 6 + 3 + a]);
        }
    return 0;
}

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
