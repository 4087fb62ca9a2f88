// internal.hpp -- shared declarations of the MI355X libcwipc_util implementation.
//
// Layering:
//   logging.cpp     cwipc_log & friends            (reference src/logging.cpp)
//   device.cpp      device selection, per-thread stream, memory pool, profiling
//   pointcloud.cpp  cwipc_hip_pointcloud container, C accessors, packet / dump I/O
//   synthetic.cpp   cwipc_synthetic source          (reference src/cwipc_synthetic.cpp)
//   stubs.cpp       out-of-scope constructors that fail loudly
//   filters.cpp     C entry points of the hot path (compaction, exact filters, join, downsample, SOR, direction), host orchestration
//   registration.cpp  C entry points of the registration tooling: distances, KDE, ICP, the floor and tile helpers, bounds
//   render.cpp      C entry points of the renderer and the marker detector
//   entry.hpp       how those three resolve and wrap their clouds
//   codec_encode.cpp  cwipc_hip_new_encoder / _encodergroup: the octree codec, packets out
//   codec_decode.cpp  cwipc_hip_new_decoder: the octree codec, packets in
//   codec_host.cpp    the codec's entry points that never touch the GPU: packet information and the host conversions
//   codec_stage.hpp   the structs the codec's kernels are handed and the staging arithmetic that fills them (free of HIP)
//   codec_shared.hpp  what the encoder and the decoder share on the host
//   c_boundary.hpp    the guards of the C boundary that the codec's and the RGB-D source's entries share
//   rgbd.cpp        cwipc_hip_from_rgbd and its two mappings: the RGB-D source end for aligned images (images in, device-resident cloud out)
//   rgbd_rig.cpp    cwipc_hip_rgbd_rig_*: the same for raw sensor pairs, a rig's create, grabs, history and queries
//   rgbd_stage.hpp  the structs the RGB-D kernels are handed, the refusals, a grab's plan and every device block's carve (free of HIP)
//   rgbd_shared.hpp what rgbd.cpp and rgbd_rig.cpp share on the host: uploads, the finished cloud, the attached images
//   kernels_*.hip   the HIP kernels (gfx950)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstddef>
#include <atomic>
#include <memory>
#include <utility>
#include <mutex>
#include <string>
#include <vector>

#include "cwipc_util/api.h"
#include "cwipc_util_amd/hip_ext.h"
#include "pinned_report.hpp"
#include "codec_stage.hpp"
#include "rgbd_stage.hpp"   // (with the four RGB-D terms headers)

// ---------------------------------------------------------------------------
// logging (reference include/cwipc_util/internal/logging.hpp:11-21)
// ---------------------------------------------------------------------------
extern "C" {
_CWIPC_UTIL_EXPORT void cwipc_log(cwipc_log_level level, std::string module, std::string message);
_CWIPC_UTIL_EXPORT void cwipc_log_set_errorbuf(char **errorbuf);
_CWIPC_UTIL_EXPORT cwipc_log_level cwipc_log_get_level();
}

namespace cwipc_amd {

// Reject a constructor call whose apiVersion is outside the accepted window
// (pattern of reference src/cwipc_util.cpp:663-670).  Returns true if rejected.
bool api_version_rejected(const char *fname, uint64_t apiVersion, char **errorMessage);

// ---------------------------------------------------------------------------
// device context
// ---------------------------------------------------------------------------

// Record a HIP failure: thread-local text + cwipc_log(ERROR).  Returns false.
bool hip_failed(hipError_t err, const char *what, const char *file, int line);
// The same for a call that was turned away before it reached the device (bad arguments): the text cwipc_hip_last_error() returns.
void note_error(const char *who, const std::string &message);
#define CW_HIP_OK(expr) ((expr) == hipSuccess ? true : ::cwipc_amd::hip_failed(hipGetLastError(), #expr, __FILE__, __LINE__))
#define CW_HIP_TRY(expr)                                                            \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess) {                                                     \
            ::cwipc_amd::hip_failed(_e, #expr, __FILE__, __LINE__);                 \
            return false;                                                           \
        }                                                                           \
    } while (0)

// True when a usable GPU exists; logs an ERROR (once per call) otherwise.  The
// product has NO CPU fallback for the filters: callers return NULL when false.
bool device_available(const char *who);
int current_device();

// Device memory pool: size-classed free lists, never shrinks unless trimmed.
// Library calls synchronise their stream before returning, so a block can be reused by any
// stream as soon as it has been released.  The one exception is a filter result whose last
// kernel is still in flight when the call returns: it carries a `ready` event (DeviceSoA),
// consumers make their stream wait for it, and its block is released only after the event.
void *pool_alloc(size_t bytes);
void pool_free(void *ptr);

struct PoolDeleter {
    void operator()(void *p) const { pool_free(p); }
};

// Per-thread execution context: one non-blocking stream, pinned staging, scratch.
struct ThreadCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    // A second stream: cwipc_downsample alternates between the two (with a workspace for each), so that the
    // finalize kernel of one call, in flight when the call returns, does not hold up the first kernel of
    // the next.  Everything else runs on `stream`; sync() waits for both.
    hipStream_t stream_alt = nullptr;
    // ... and a third and fourth (r4), created when a thread's downsample calls come faster than two workspaces turn around
    static constexpr int EXTRA_STREAMS = 2;
    hipStream_t stream_extra[EXTRA_STREAMS] = {nullptr, nullptr};
    hipStream_t extra_stream(int i);   // stream_extra[i], created on first use (nullptr on failure)
    void *pinned = nullptr;       // staging for H2D/D2H of AoS points
    size_t pinned_bytes = 0;
    uint32_t *host_words = nullptr;   // 64 pinned 32-bit words for small read-backs
    void *dev_words = nullptr;        // 64 device words
    uint32_t *tickets = nullptr;      // 16 device words, zero between kernels: "last workgroup done" counters (each kernel that uses one sets it back)
    void *scratch = nullptr;          // device scratch of this thread's calls (block counts of a compaction): work on one
    size_t scratch_bytes = 0;         //   stream is ordered, so the next call may overwrite it while nobody else can
    uint32_t tag = 0;                 // sequence number of the last value a kernel published into host_words
    // host_words as 64-bit report words under `tag` (pinned_report.hpp)
    PinnedReport report() { return PinnedReport(reinterpret_cast<volatile unsigned long long *>(host_words), tag); }
    void *device_scratch(size_t bytes);
    std::vector<void *> deferred;     // pool blocks whose last kernel may still run: given back at the next sync()
    void free_later(void *pool_block) { if (pool_block) deferred.push_back(pool_block); }
    bool ensure();                    // create the stream etc. for the current device
    void *staging(size_t bytes);      // pinned buffer of at least `bytes`
    bool sync();
    ~ThreadCtx();
};
ThreadCtx &tctx();

// How long a call polls pinned memory for a kernel's report before it falls back to an ordinary stream wait
// (microseconds; CWIPC_POLL_US overrides, 0 = never poll: the test suite runs both ways).
inline long poll_budget_us() {
    const char *e = getenv("CWIPC_POLL_US");
    return e ? atol(e) : 2000;
}

// Cached hipEvents without timing, for the `ready` marks of asynchronous results.
hipEvent_t event_get();
void event_put(hipEvent_t e);

// Profiling: kernels are launched through CW_LAUNCH so that per-kernel device
// time can be collected with hipEvents on the launching stream.
void profile_begin(const char *name, hipStream_t s);
void profile_end(hipStream_t s);
void profile_collect();   // after a stream sync: fold finished event pairs into totals
bool profiling_enabled();

#define CW_LAUNCH(name, kernel, grid, block, shmem, stream, ...)                               \
    do {                                                                                       \
        if (::cwipc_amd::profiling_enabled()) ::cwipc_amd::profile_begin(name, stream);        \
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                   \
        if (::cwipc_amd::profiling_enabled()) ::cwipc_amd::profile_end(stream);                \
    } while (0)

// ---------------------------------------------------------------------------
// point storage
// ---------------------------------------------------------------------------

// A pool block that several clouds may hold (clouds are immutable: a filter that changes colours or tiles only
// gives its result the input's coordinate planes instead of copying them).
struct PlaneBlock {
    void *ptr = nullptr;
    explicit PlaneBlock(void *p) : ptr(p) {}
    PlaneBlock(const PlaneBlock &) = delete;
    PlaneBlock &operator=(const PlaneBlock &) = delete;
    ~PlaneBlock() { if (ptr) pool_free(ptr); }
};

// Device representation: four planes, each `stride` elements long (stride = npoints rounded up to 256, so every
// plane starts on a 1 KiB boundary and a full wave step of 256 points can always be loaded): x, y, z in one pool
// block, rgbt in another.  rgbt = r | g<<8 | b<<16 | tile<<24, i.e. the last four bytes of a cwipc_point read as
// one little-endian word.
struct DeviceSoA {
    std::shared_ptr<PlaneBlock> xyz_block, rgbt_block;
    size_t npoints = 0;
    size_t stride = 0;
    int device = 0;
    // The cloud's first point, when the host knows it (the octree lattice of cwipc_downsample is
    // anchored there); fetched from the device on demand otherwise.
    mutable bool has_first = false;
    mutable float first[3] = {0, 0, 0};
    // Which tile values MAY occur in the cloud (bit t of 256), when a producer knows: a tilemap with one target value, a tile
    // filter's result, the synthetic source, a census (cwipc_hip_tiles_used); filters that keep the tile words hand it on,
    // a join takes the union.  A one-element set on a cloud with points says that EVERY point has that tile: cwipc_tilefilter
    // for it hands the planes on without looking at a point (a camera's tile is filtered by its own mask in the per-tile chain
    // of the reference, python/cwipc/registration/util.py:170-182), and a filter for a value outside the set is empty.
    // Producers fill the set before they publish the cloud; a census (cwipc_hip_tiles_used) adds it to a cloud other threads may be
    // filtering at that moment: the words first, then the flag with release order, and readers take the flag with acquire order.
    mutable std::atomic<bool> has_tiles{false};
    mutable uint32_t tiles[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void set_tiles(const uint32_t words[8]) const { for (int i = 0; i < 8; i++) tiles[i] = words[i]; has_tiles.store(true, std::memory_order_release); }
    void set_tiles_from(const DeviceSoA &o) const { if (o.has_tiles.load(std::memory_order_acquire)) set_tiles(o.tiles); else has_tiles.store(false, std::memory_order_release); }
    void set_one_tile(unsigned t) const { uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0}; w[(t & 255u) >> 5] = 1u << (t & 31u); set_tiles(w); }
    bool may_have_tile(unsigned t) const { return !has_tiles.load(std::memory_order_acquire) || t > 255u || ((tiles[t >> 5] >> (t & 31u)) & 1u) != 0u; }
    bool only_tile(unsigned t) const {
        if (!has_tiles.load(std::memory_order_acquire) || t > 255u) return false;
        for (int i = 0; i < 8; i++) if (tiles[i] != (i == (int)(t >> 5) ? 1u << (t & 31u) : 0u)) return false;
        return true;
    }
    // Set (before the cloud is published) when the producing call returned with its last kernel
    // still running: every consumer orders its stream after this event; never changed afterwards.
    hipEvent_t ready = nullptr;
    void mark_pending(hipStream_t producer);            // record `ready` on the producer's stream
    void wait_on(hipStream_t consumer) const {          // device-side wait, no host blocking
        if (ready && hipStreamWaitEvent(consumer, ready, 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipEventSynchronize(ready);           // order on the host instead
        }
    }
    void wait_host() const {                            // for consumers outside the library's streams
        if (ready) (void)hipEventSynchronize(ready);
    }
    // The other direction: a call that returned with a kernel still READING these planes leaves an event
    // here (one per stream, the latest), and the planes are not given back to the pool before it.
    mutable std::mutex readers_mutex;
    mutable std::vector<std::pair<hipStream_t, hipEvent_t>> readers;
    void note_reader(hipStream_t consumer) const;
    float *x() const { return (float *)xyz_block->ptr; }
    float *y() const { return (float *)xyz_block->ptr + stride; }
    float *z() const { return (float *)xyz_block->ptr + 2 * stride; }
    uint32_t *rgbt() const { return (uint32_t *)rgbt_block->ptr; }
    ~DeviceSoA() {
        if (ready) {
            (void)hipEventSynchronize(ready);   // normally long complete
            event_put(ready);
        }
        for (auto &r : readers) {
            (void)hipEventSynchronize(r.second);
            event_put(r.second);
        }
        // (the blocks go back to the pool when the last cloud that holds them has come this far)
    }
};
std::shared_ptr<DeviceSoA> soa_alloc(size_t npoints);
// A cloud with `src`'s coordinates (the very planes) and colour / tile words of its own, still to be written.
std::shared_ptr<DeviceSoA> soa_with_new_rgbt(const std::shared_ptr<DeviceSoA> &src);
// ... and the other way round: `src`'s colour / tile words, coordinate planes of its own.
std::shared_ptr<DeviceSoA> soa_with_new_xyz(const std::shared_ptr<DeviceSoA> &src);
// A cloud that holds `src`'s planes, all four (clouds are immutable): its blocks, count, stride and device, nothing else of it.
std::shared_ptr<DeviceSoA> share_planes(const DeviceSoA &src);
// A result of `kept` points at the front of planes with room for `room` stays in them when it uses a sixteenth of the room or more.
inline bool soa_keeps_planes(size_t kept, size_t room) { return kept * 16 >= room; }
// The result that is the first `kept` points of `dst` (room: dst->npoints): dst itself with its count shrunk -- the planes keep their
// spacing (stride) -- or, when few survive, planes of their own size, copied on the calling thread's stream and waited for.  What
// writes `dst` must be complete before the copy: the caller has waited.  nullptr: out of memory, or the copy failed (logged as `what`).
std::shared_ptr<DeviceSoA> soa_keep(const std::shared_ptr<DeviceSoA> &dst, size_t kept, const char *what);

// A filter result that is still being computed when the call returns: its planes exist, its point count does not yet.
// cwipc_downsample (octree path) hands these out in a stream of frames, so that the host does not stand between one
// frame's kernels and the next one's; the first accessor that needs the points settles it (waits, and runs the pass
// again the slow way in the rare case that its assumptions did not hold).
struct DeferredResult {
    virtual ~DeferredResult() {}
    // Blocks until the result is there; nullptr = the filter failed (logged).  May be called from any thread, any
    // number of times.
    virtual std::shared_ptr<DeviceSoA> settle() = 0;
    // Results whose timestamp and cellsize are themselves part of what is still being computed (the multi-GPU join: the
    // minimum over the ranks' clouds) hand them over here, after settle(); false = they were known when the result was made.
    virtual bool late_metadata(uint64_t *timestamp, float *cellsize) { (void)timestamp; (void)cellsize; return false; }
};

// Host memory for point buffers: page-locked and pooled when a GPU is there (the DMA engines then
// read and write it directly, no staging copy), plain malloc otherwise.
void *host_alloc(size_t bytes, bool *pinned);
void host_free(void *ptr, bool pinned);
// memcpy split over a few threads for buffers of a megabyte and more (one core copies at 10-20 GB/s)
void parallel_memcpy(void *dst, const void *src, size_t bytes);
// [ptr, ptr + bytes) in page-locked memory the CALLER holds (cwipc_hip_host_alloc / cwipc_hip_host_register): the address a kernel
// reaches it under; nullptr for any other memory
void *host_range_device_alias(const void *ptr, size_t bytes);

// Host representation: AoS exactly as handed in through the C-ABI.
struct HostAoS {
    cwipc_point *points = nullptr;
    size_t npoints = 0;
    bool pinned = false;
    ~HostAoS() { host_free(points, pinned); }
};

// The cwipc_pointcloud implementation.  Either representation may be missing;
// the other one is materialised on demand (device: filters; host: accessors).
class cwipc_hip_pointcloud : public cwipc_pointcloud {
public:
    cwipc_hip_pointcloud();
    ~cwipc_hip_pointcloud() override;

    // cwipc_pointcloud interface
    void free() override;
    cwipc_pointcloud *_shallowcopy() override;
    uint64_t timestamp() override;
    float cellsize() override;
    void _set_cellsize(float cellsize) override;
    void _set_timestamp(uint64_t timestamp) override;
    int count() override;
    size_t get_uncompressed_size() override;
    int copy_uncompressed(struct cwipc_point *pointbuf, size_t size) override;
    size_t copy_packet(uint8_t *packet, size_t size) override;
    cwipc_pcl_pointcloud access_pcl_pointcloud() override;
    cwipc_metadata *access_metadata() override;

    // construction helpers
    int from_points(const cwipc_point *points, size_t size, int npoint, uint64_t timestamp, bool exact_size = true);
    void adopt_device(std::shared_ptr<DeviceSoA> dev, uint64_t timestamp, float cellsize, bool exact_size = false);
    void adopt_deferred(std::shared_ptr<DeferredResult> pending, uint64_t timestamp, float cellsize, bool late_metadata = false);
    // What a library thread needs of this cloud to work on it after the caller has gone on (or freed the cloud): the planes, or
    // the pending result that will become them.  A cloud that lives in host memory only is uploaded first (by the caller).
    struct Snapshot {
        std::shared_ptr<DeferredResult> pending;
        std::shared_ptr<DeviceSoA> dev;
        uint64_t timestamp = 0;
        float cellsize = 0;
        bool has_data = false;
    };
    Snapshot snapshot();

    // residency
    std::shared_ptr<DeviceSoA> device_points();   // uploads if needed; nullptr on failure
    std::shared_ptr<HostAoS> host_points();       // downloads if needed; nullptr on failure
    bool has_device() { settle(); return (bool)m_dev; }
    bool has_host() { settle(); return (bool)m_host; }
    bool drop_host();
    size_t npoints() { settle(); return m_npoints; }
    bool has_data() const { return m_has_data; }

private:
    int copy_impl(struct cwipc_point *pointbuf, size_t size, bool exact, bool dst_pinned = false);
    void settle();                // a deferred result becomes an ordinary device cloud (no-op otherwise)
    std::shared_ptr<DeferredResult> m_pending;
    std::mutex m_lock;
    uint64_t m_timestamp = 0;
    float m_cellsize = 0;
    size_t m_npoints = 0;
    bool m_has_data = false;      // counts towards cwipc_dangling_allocations
    bool m_exact_size = false;    // from_points flavour: copy_uncompressed wants size == exact
    bool m_late_metadata = false; // timestamp and cellsize come with the pending result
    std::shared_ptr<HostAoS> m_host;
    std::shared_ptr<DeviceSoA> m_dev;
    cwipc_metadata *m_metadata = nullptr;
};

// A cwipc_pointcloud that is not ours (another library's implementation) is
// read through its virtual interface into a temporary of ours.
std::unique_ptr<cwipc_hip_pointcloud> import_foreign(cwipc_pointcloud *pc);
cwipc_hip_pointcloud *as_ours(cwipc_pointcloud *pc);

void count_alloc();
void count_dealloc();

// ---------------------------------------------------------------------------
// kernel launchers (kernels_basic.hip, kernels_voxel.hip, kernels_sor.hip, kernels_direction.hip, kernels_nn.hip, kernels_kde.hip, kernels_icp.hip,
// kernels_floor.hip, kernels_render.hip, kernels_markers.hip, kernels_cluster.hip;
// the point grid they search on: point_grid.hpp, kernels_grid.hip)
// All work on the calling thread's stream; none synchronises unless stated.
// ---------------------------------------------------------------------------
struct PlaneRule;   // plane_seg_terms.hpp

namespace k {

// AoS (device) <-> SoA
void aos_to_soa(const cwipc_point *aos, const DeviceSoA &dst, size_t n, hipStream_t s);
constexpr int MAX_SLOTS = 64;
void slots_to_soa(const void *slots, int nslots, size_t slot_rows, size_t header_rows, const uint32_t *counts, const DeviceSoA &dst, hipStream_t s);
void soa_to_aos(const DeviceSoA &src, cwipc_point *aos, size_t n, hipStream_t s);

// Stable compaction.  mode 0: tile == 0 || tile == pt.tile ; mode 1: half-open bbox ;
// mode 2: (pt.tile & tile) != 0 ; mode 3: !(dist[i] > thr)  (outlier removal).
struct Predicate {
    int mode;
    int tile;
    float bbox[6];
    const float *dist;
    double thr;
    const double *thr_dev;   // mode 3: device address of the threshold when a kernel computed it (thr is ignored then)
    // mode 3, small clouds (r4): the threshold is still 1024 pairs of partial sums (sor_stats_partial_device): the count kernel's workgroups run the
    // statistics' tree themselves -- each the same tree -- and the first one writes the threshold to thr_out (= thr_dev) for the scatter kernel
    const double *stat_partial;
    size_t stat_n;
    float stat_mul;
    double *thr_out;
};
// Pass 1: per-block keep counts into block_counts[nblocks]; returns nblocks through the argument.
size_t compact_blocks(size_t n);
size_t compact_small_cloud_limit();   // clouds up to here go through compact_count_scan
void compact_count(const DeviceSoA &src, const Predicate &p, uint32_t *block_counts, hipStream_t s);
// count and scan in one launch (the last workgroup to finish scans the block counts): for clouds of up to a million points,
// where a launch costs the host more than the kernel costs the device; `ticket`: a zeroed device word, left zeroed
bool compact_count_scan(const DeviceSoA &src, const Predicate &p, uint32_t *block_counts, uint32_t *ticket, unsigned long long *total_host, uint32_t tag,
                        hipStream_t s);
// Exclusive scan of block_counts in place; total written to *total_dev.
void compact_scan(uint32_t *block_counts, size_t nblocks, unsigned long long *total_host, uint32_t tag, hipStream_t s);
// Pass 2: scatter kept points to dst in input order.
// total_host != nullptr: block_offsets are the count kernel's COUNTS; every workgroup sums those in front of it, the first one publishes the total
void compact_scatter(const DeviceSoA &src, const Predicate &p, const uint32_t *block_offsets, const DeviceSoA &dst, hipStream_t s,
                     unsigned long long *total_host = nullptr, uint32_t tag = 0);

// Per-point maps on the rgbt word (x,y,z copied).
void map_tile(const DeviceSoA &src, const DeviceSoA &dst, const uint8_t *dev_map256, hipStream_t s);
void map_color_bits(const DeviceSoA &src, const DeviceSoA &dst, uint32_t clearBits, uint32_t setBits, hipStream_t s);
// mode 0: p' = R p + t with m = rows of [R | t]; mode 1: p' = (p + (m[3], m[7], m[11])) * m[0]; f64 arithmetic, one rounding to fp32
void map_affine(const DeviceSoA &src, const DeviceSoA &dst, const double m[12], int mode, hipStream_t s);
// the synthetic source's cloud written straight into device planes; the tables are device memory (see synthetic.cpp)
void synthetic_fill(const DeviceSoA &dst, int hsteps, int asteps, float m_angle, bool eyes_white, const float *radius, const float *height,
                    const float *angle, const double *sin_a, const double *cos_a, hipStream_t s);
// simulatecams (hard): tile = 1 << index of the camera direction (dirs: cos, sin per camera) nearest to the centred position
void map_cameras(const DeviceSoA &src, const DeviceSoA &dst, int ncam, float cen_x, float cen_z, const double *dirs, hipStream_t s);
// simulatecams (soft): the nearest or the second nearest direction, by one draw per point of the stream of `seed` (counter_rng.hpp); ncam >= 2
void map_cameras_soft(const DeviceSoA &src, const DeviceSoA &dst, int ncam, float cen_x, float cen_z, const double *dirs, double skew, uint64_t seed,
                      hipStream_t s);
// the noise filter: p' = p + a random vector of length up to `distance`, four draws per point of the stream of `seed` (counter_rng.hpp)
void map_noise(const DeviceSoA &src, const DeviceSoA &dst, double distance, uint64_t seed, hipStream_t s);
// ORs the set of tile values that occur into 8 device words
void tiles_used(const DeviceSoA &src, uint32_t *dev_bits8, hipStream_t s);
// first256[t] = index of the first point with tile value t, 0xffffffff if there is none (256 device words)
void tile_first_index(const DeviceSoA &src, uint32_t *dev_first256, hipStream_t s);
// colorize: dev_table = 256 entries of {double cw[3]; double valid;} followed by 256 doubles old/255.0, then (1-w).
void map_colorize(const DeviceSoA &src, const DeviceSoA &dst, const double *dev_table, hipStream_t s);

// Concatenate nsrc clouds (device array of plane pointers) into dst.
struct JoinPart {
    const float *x, *y, *z;
    const uint32_t *rgbt;
    size_t n;
    size_t dst_offset;
};
void join_copy(const JoinPart &part, const DeviceSoA &dst, hipStream_t s);

// ---- kernels_floor.hip: the floor and tile helpers of the registration pipeline (python/cwipc/registration/util.py:146-229) ----
// A point is floor iff (double)y < level.  Class A of the partition comes first in the output, class B behind it, both in
// input order: A = floor points (FLOOR_KEEP_FLOOR), with FLOOR_LIMIT_RADIUS only those with (double)d < radius, d the float32
// norm of (x, y, z); B = the other points (FLOOR_KEEP_REST).
struct FloorArgs {
    double level;
    double radius;
    int flags;   // CWIPC_HIP_FLOOR_* of hip_ext.h
};
constexpr int FLOOR_KEEP_FLOOR = CWIPC_HIP_FLOOR_KEEP_FLOOR, FLOOR_KEEP_REST = CWIPC_HIP_FLOOR_KEEP_REST, FLOOR_LIMIT_RADIUS = CWIPC_HIP_FLOOR_LIMIT_RADIUS;
size_t floor_blocks(size_t n);
// counts: 2 * floor_blocks(n) + 2 device words -- per-workgroup counts of A, then of B; the scan turns both into offsets, leaves the
// totals in the last two words and in two pinned 64-bit host words (the count below `tag`); the scatter writes dst (A + B points)
void floor_count(const DeviceSoA &src, const FloorArgs &a, uint32_t *counts, hipStream_t s);
void floor_scan(uint32_t *counts, size_t nblocks, unsigned long long *total_host, uint32_t tag, hipStream_t s);
void floor_scatter(const DeviceSoA &src, const FloorArgs &a, const uint32_t *offsets, const DeviceSoA &dst, hipStream_t s);
// out_rgbt[j] for j < n_first: rgbt[j]'s colour with the tile byte of rgbt[perm[j]], perm the stable ascending argsort of the
// splitmix64 keys of seed; for j >= n_first a copy.  The scratch blocks are freed at the calling thread's next sync().
bool floor_shuffle(const uint32_t *rgbt, size_t n_first, size_t n, uint64_t seed, uint32_t *out_rgbt, hipStream_t s);
// Exact radix selection per class (0 floor, 1 rest) on d = sqrt((x*x + 0) + z*z): state (floor_radius_state_bytes() of device
// memory) ends with the two class counts in words 0-1 and sorted(d)[lo], sorted(d)[min(lo + 1, n - 1)] per class as float bits
// in words 2-5 (NaN for an empty class), lo = floor((n - 1) * 0.99f) in float32 as numpy.percentile computes it.
size_t floor_radius_state_bytes();
void floor_radius_select(const DeviceSoA &src, double level, uint32_t *state, hipStream_t s);
// counts of the tile byte (256 x 64 bit, device), optionally of the non-floor points only
void tile_histogram(const DeviceSoA &src, int nonfloor_only, double level, unsigned long long *dev_counts256, hipStream_t s);
// per workgroup min x, y, z, max x, y, z (NaN skipped per coordinate; +inf / -inf where there is nothing): bounds_blocks(n) x 6 floats
unsigned bounds_blocks(size_t n);
void bounds_partial(const DeviceSoA &src, float *partial, hipStream_t s);
// The same partition with RULE S's classes (hip_ext.h): A = the inliers of a plane (PLANE_KEEP_INLIERS; with PLANE_BELOW_IS_INLIER
// everything with e <= distance), B = the other points (PLANE_KEEP_REST).
struct PlaneArgs {
    double plane[4];
    double distance;
    int flags;   // CWIPC_HIP_PLANE_KEEP_* and CWIPC_HIP_PLANE_BELOW_IS_INLIER of hip_ext.h
};
void floor_count(const DeviceSoA &src, const PlaneArgs &a, uint32_t *counts, hipStream_t s);
void floor_scatter(const DeviceSoA &src, const PlaneArgs &a, const uint32_t *offsets, const DeviceSoA &dst, hipStream_t s);

// ---- kernels_plane.hip: the plane search of RULE S (hip_ext.h; the arithmetic is plane_seg_terms.hpp's) ----
constexpr int PLANE_SCORE_TILE = 2048;    // points a workgroup of the score kernel holds in registers at a time
constexpr int PLANE_SCORE_GRID = 512;     // its largest grid.x: workgroup (x, y) takes tiles x, x + grid.x, ...
constexpr int PLANE_SCORE_HBLOCK = 64;    // hypotheses whose counts it keeps in LDS at a time: blocks y, y + grid.y, ...
// What plane_best leaves in device memory and the refit adds its sums to: one read-back for both.
struct PlaneBest {
    double plane[4];
    double anchor[3];
    uint32_t h, count, nvalid, found;
    uint32_t triple[3], pad;
    unsigned long long sums[10];
};
// One pool block: the table (planes 4 H doubles, triples 3 H words, valid H words, counts H words), the best record, the score
// kernel's partial counts (grid x H words).
struct PlaneWork {
    double *planes = nullptr;
    uint32_t *triples = nullptr, *valid = nullptr, *counts = nullptr, *partial = nullptr;
    PlaneBest *best = nullptr;
    unsigned grid = 1;
};
unsigned plane_score_grid(size_t n, uint32_t H);
size_t plane_work_bytes(size_t n, uint32_t H);
void plane_work_layout(void *block, size_t n, uint32_t H, PlaneWork &w);
// No wait in any of them.  The table of the rule's H hypotheses:
void plane_hypotheses(const DeviceSoA &src, const PlaneRule &r, const PlaneWork &w, hipStream_t s);
// counts[0, H) of the table's valid rows -- or, with `one`, counts[0] of that plane alone (the recount)
void plane_score(const DeviceSoA &src, double distance, uint32_t H, const PlaneWork &w, const double *one, hipStream_t s);
// the best record from table and counts (its sums zeroed) ...
void plane_best(const DeviceSoA &src, uint32_t H, const PlaneWork &w, hipStream_t s);
// ... and the refit's sums over the best hypothesis' inliers, added to it (nothing when found == 0)
void plane_refit_sums(const DeviceSoA &src, double distance, const PlaneWork &w, hipStream_t s);

// ---- kernels_render.hip: cwipc_hip_render (the contract is at the top of that file and in hip_ext.h) ----
struct RenderArgs {
    int width, height;
    int half;        // (point_size - 1) / 2
    int tilemask;
    double fx, fy, cx, cy, near_z, far_z;
    double e[12];    // rows 0-2 of the world -> camera matrix
};
// keys: width * height 64-bit words (float_bits(depth) << 32 | index, all ones: nothing).  fill also zeroes *covered, which resolve
// counts the covered pixels into.  resolve writes depth (npix floats), rgb (3 npix bytes, 16-byte aligned) and index (npix words,
// or nullptr); rgbt is only read for covered pixels.
void render_fill(unsigned long long *keys, size_t npix, uint32_t *covered, hipStream_t s);
void render_splat(const DeviceSoA &src, const RenderArgs &a, unsigned long long *keys, hipStream_t s);
void render_resolve(const unsigned long long *keys, const uint32_t *rgbt, size_t npix, uint32_t background, float *depth, uint8_t *rgb, int32_t *index,
                    uint32_t *covered, hipStream_t s);

// ---- kernels_markers.hip: cwipc_hip_detect_markers (the contract is at the top of that file and in hip_ext.h) ----
constexpr int MARKER_MAX_SIDE = 8192;   // (derived at the top of kernels_markers.hip)
// What the decode kernel leaves per candidate: id -1 when it is no marker; the corners in output order, the depth image's value at them
struct MarkerRecord {
    int32_t id;
    uint32_t area, label;
    int32_t x[4], y[4];
    float depth[4];
    uint32_t pad;
};
struct MarkerWorkspace {
    bool ok = false;
    const uint32_t *ncand = nullptr;       // the number of candidates (device)
    const MarkerRecord *records = nullptr; // that many records (device), in no particular order
    const uint32_t *label = nullptr;       // per pixel its component's label, 0xFFFFFFFF for a light pixel (device)
    uint32_t cap = 0;                      // the bound on the number of candidates
};
size_t marker_workspace_bytes(size_t npix, int min_side, int nmarkers);
// All of the detector's kernels on stream s, nothing waited for.  dev_rgb: the image on the device; dict_staged: the dictionary in
// pinned host memory that stays as it is until the stream has been waited for; dev_depth: a depth image for the records, or nullptr;
// workspace: marker_workspace_bytes() of device memory.  The parameters have been checked.
MarkerWorkspace marker_launch(const uint8_t *dev_rgb, int width, int height, const uint32_t *dict_staged, int nmarkers, const cwipc_hip_marker_params &p,
                              const float *dev_depth, void *workspace, hipStream_t s);
void marker_labels_out(const uint32_t *label, size_t npix, int32_t *out, hipStream_t s);

// ---- kernels_rgbd.hip: cwipc_hip_from_rgbd (the contract is in rgbd_terms.hpp and hip_ext.h) ----
// (RgbdCamDev, one camera of a frame as the kernels see it: rgbd_stage.hpp)
size_t rgbd_blocks(uint32_t total_pixels);
// Pass 1: per workgroup the number of pixels that give a point, then the exclusive scan of those: counts (rgbd_blocks() + 1 device
// words) ends up holding offsets and the total, which also goes to *total_host (pinned) below `tag`.  Frames of up to 256 k pixels:
// one launch, the last workgroup scans (ticket: a zeroed device word, left zeroed); larger ones: the count kernel, then compact_scan.
void rgbd_count(const RgbdCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, uint32_t *counts, uint32_t *ticket,
                unsigned long long *total_host, uint32_t tag, hipStream_t s);
// Pass 2: the points, in pixel order, into dst (room for total_pixels points).
void rgbd_scatter(const RgbdCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, const uint32_t *offsets, const DeviceSoA &dst,
                  hipStream_t s);
// ---- the raw entry, cwipc_hip_rgbd_rig_grab (the contract is in rgbd_lens.hpp and hip_ext.h) ----
// (RgbdRawCamDev, one camera of a rig: rgbd_stage.hpp)
void rgbd_count(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, uint32_t *counts, uint32_t *ticket,
                unsigned long long *total_host, uint32_t tag, hipStream_t s);
void rgbd_scatter(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, const uint32_t *offsets, const DeviceSoA &dst,
                  hipStream_t s);
// Box erosion of every camera's depth image in place, 0 <= ex, ey <= 32: two launches over the word grid (total_words words).
void rgbd_erode(const RgbdRawCamDev *cams, int ncam, uint32_t total_words, int ex, int ey, unsigned long long *words, hipStream_t s);
// Every depth pixel's registered colour; the depth of a pixel without one is cleared.
void rgbd_register(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, hipStream_t s);
// The occlusion test (rgbd_lens.hpp), between erosion and count in place of rgbd_register.  zbuf: one word per colour pixel of every
// camera, all ones.  rgbd_zsplat: every candidate's key goes, by atomic minimum, to the cell of its own colour pixel.
// rgbd_register_occluded: rgbd_register, with Zmin at a candidate's colour pixel taken as the smallest word of its (2 splat + 1)^2
// square inside the colour image, an occluded candidate being a pixel without a colour.
// The depth post-processing (rgbd_depthfilter.hpp), in front of the erosion.  rgbd_spatial: `magnitude` iterations of rows forward and
// backward, then columns forward and backward, in place: two launches per iteration.  rgbd_temporal: the per-pixel update of the
// depth images and of the rig's state (value, history: one entry per depth pixel of the frame, numbered through as the pixels are).
void rgbd_spatial(const RgbdRawCamDev *cams, int ncam, uint32_t row_groups, uint32_t col_groups, int magnitude, const RgbdSmoothTerms &t, hipStream_t s);
uint32_t rgbd_line_groups(uint32_t lines);
void rgbd_temporal(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, const RgbdSmoothTerms &t, int persistency, double *value, uint8_t *history,
                   hipStream_t s);
void rgbd_zsplat(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, unsigned long long *zbuf, hipStream_t s);
// Decimation and hole filling (rgbd_decimate.hpp).  rgbd_decimate: every camera's full_depth, k = 2 .. 8, into its depth_rw, in front
// of everything else; tiles: the sum of rgbd_decimate_tiles(width, height) over the cameras (the decimated sizes).
// rgbd_holefill: rule 0c, mode 1 .. 3, in place as far as the caller sees; rows: the sum of the cameras' heights; scratch: total_pixels
// depth values (modes 2 and 3 only: they write it from the images and then copy it back, two launches).
uint32_t rgbd_decimate_tiles(uint32_t width, uint32_t height);
void rgbd_decimate(const RgbdRawCamDev *cams, int ncam, int k, uint32_t tiles, hipStream_t s);
void rgbd_holefill(const RgbdRawCamDev *cams, int ncam, int mode, uint32_t rows, uint32_t total_pixels, uint16_t *scratch, hipStream_t s);
void rgbd_register_occluded(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, const unsigned long long *zbuf, int splat, double margin,
                            hipStream_t s);

// ---- kernels_codec.hip: the octree codec (RULE C: hip_ext.h; the arithmetic: codec_terms.hpp) ----
// What the bounds leave on the device and the host reads back with nodes[]: the cube and the number of points that take part.
struct CodecCube {
    float mn[3];
    uint32_t nfinite;
    double side;
};
// what a workgroup of the bounds kernel leaves of its points: the box of the finite ones and their number
struct CodecBounds {
    float lo[3], hi[3];
    uint32_t count, pad;
};
// (CodecLeafSum, CodecEmit, CodecDecode: codec_stage.hpp)
size_t codec_blocks(size_t n);
size_t codec_bounds_bytes(size_t n);
// the cube of the points whose coordinates are all finite; partial: codec_bounds_bytes() of device memory
void codec_cube(const DeviceSoA &src, void *partial, CodecCube *cube, hipStream_t s);
// keys and index: 2 n entries each; the sorted halves are keys + n and index + n.  A point that is left out sorts behind the cube's nfinite others.
bool codec_sort(const DeviceSoA &src, const CodecCube *cube, int bits, unsigned long long *keys, uint32_t *index, hipStream_t s);
// counts: bits rows of codec_blocks(n) + 1 words; row L ends up as the workgroups' offsets at depth L and nodes[L], which also goes to
// total_host[L] (pinned) below `tag`
void codec_count_scan(const unsigned long long *sorted_keys, size_t n, const CodecCube *cube, int bits, uint32_t *counts, unsigned long long *total_host,
                      uint32_t tag, hipStream_t s);
// the body of a packet of e.bits <= sort_bits from keys sorted at sort_bits and their scanned counts
void codec_emit(const unsigned long long *sorted_keys, const uint32_t *sorted_index, const DeviceSoA &src, const CodecCube *cube, int sort_bits,
                const uint32_t *offsets, const CodecEmit &e, int colour_shift, hipStream_t s);
size_t codec_decode_scratch_words(const CodecDecode &d);
// the leaves' keys from the occupancy bytes, depth by depth: returns ping or pong, whichever holds them (d.nleaves > 0)
unsigned long long *codec_expand(const uint8_t *occupancy, const CodecDecode &d, unsigned long long *ping, unsigned long long *pong, uint32_t *scratch,
                                 hipStream_t s);
void codec_decode(const uint8_t *occupancy, const CodecDecode &d, unsigned long long *ping, unsigned long long *pong, uint32_t *scratch, const DeviceSoA &dst,
                  hipStream_t s);

// ---- kernels_entropy.hip: the entropy-coded packet form (RULE E: hip_ext.h; the arithmetic: entropy_terms.hpp) ----
// (EntropyStreams, EntropyEncode, EntropyDecode and the encoder's work block, stage_encode_work(): codec_stage.hpp)
void entropy_encode(const EntropyEncode &e, hipStream_t s);
void entropy_decode(const EntropyDecode &d, unsigned long long *status_host, uint32_t tag, hipStream_t s);

// ---- kernels_transform.hip: transform colour coding (RULE T: hip_ext.h; the arithmetic: transform_terms.hpp) ----
// (TransformTree and its planes' layout, stage_tree_planes(): codec_stage.hpp)
size_t transform_scan_words(const TransformTree &t);
// the planes' fields from the header's counts and the quality's scale
void transform_tree_counts(TransformTree &t, int bits, const uint32_t *nodes, uint32_t nleaves, uint32_t q16);
// first[] from the occupancy bytes
void transform_prepare(const TransformTree &t, hipStream_t s);
// colours: RULE C's colour plane at 8 bits.  -> zz[], and the root's values (dc) in value[ch * (inner + nleaves)]
void transform_forward(const TransformTree &t, const uint8_t *colours, hipStream_t s);
// zz[] -> tokens (3 planes of nleaves - 1 bytes) and escapes (3 planes of escape_stride u16, zeroed by the caller); the number of
// escapes of channel ch is left in transform_escape_total(t, ch)
void transform_tokens(const TransformTree &t, uint8_t *tokens, uint16_t *escapes, uint32_t escape_stride, hipStream_t s);
const uint32_t *transform_escape_total(const TransformTree &t, int ch);
// The packet from the fixed bytes (Q16) on: what the entropy stage left in `in` (its plan, its report) for the streams occupancy,
// three token planes and the tile plane, with the escape streams put in their places.  report (device, 4 words): as EntropyEncode's.
struct TransformAssemble {
    int bits, entropy_streams;
    const uint32_t *plan, *in_report;
    const uint8_t *in;
    const uint16_t *escapes;
    uint32_t escape_stride;
    const uint32_t *escape_total[3];
    const int32_t *dc[3];
    uint32_t q16;
    uint8_t *out;
    uint64_t out_capacity;
    uint32_t *report;
};
void transform_assemble(const TransformAssemble &a, hipStream_t s);
// tokens and the raw escape streams (in + escape_offset[ch], nescapes[ch] u16 values) -> zz[]; the number of tokens equal to 255 of
// channel ch goes to totals_host[ch] (pinned) below `tag`
void transform_untoken(const TransformTree &t, const uint8_t *tokens, const uint8_t *in, const uint32_t escape_offset[3], const uint32_t nescapes[3],
                       unsigned long long *totals_host, uint32_t tag, hipStream_t s);
// weight[], then zz[] and dc -> the leaves' colours into RULE C's colour plane at 8 bits (3 nleaves bytes)
void transform_inverse(const TransformTree &t, const int32_t dc[3], uint8_t *colours, hipStream_t s);

// ---- kernels_inter.hip: inter-frame coding (RULE P: hip_ext.h; the arithmetic: inter_terms.hpp) ----
// A frame's leaves as a decoder has them: keys ascending, the stored colours as three byte planes of n, the tiles.
struct InterLeavesDev {
    unsigned long long *keys;
    uint8_t *colour, *tiles;   // colour + ch * n
    uint32_t n;
};
// What the cube kernel leaves behind the cube for the one read-back.
struct InterCubeReport {
    CodecCube cube;
    uint32_t delta, pad;       // 1: the frame is contained in the GOP's cube, which is now `cube`
};
// After codec_cube: the frame's cube becomes the GOP's cube where `allow_delta` and the frame is contained in it (delta), else the
// frame's own cube grown by exp_factor (key).  One wave.
void inter_cube(const void *partial, size_t npoints, InterCubeReport *report, bool allow_delta, const float gop_mn[3], double gop_side, float exp_factor,
                hipStream_t s);
// The leaves of the packet body that codec_emit made from keys sorted at e.bits: keys compacted, colours unpacked, tiles copied.
void inter_leaves_of_body(const unsigned long long *sorted_keys, size_t npoints, const CodecCube *cube, const uint32_t *offsets, const CodecEmit &e,
                          int colour_bits, const InterLeavesDev &out, hipStream_t s);
// The same from a decoder's body: the keys are there already (out.keys), tiles == nullptr: tile_value throughout.
void inter_leaves_of_planes(const uint32_t *colours, uint64_t colour_words, const uint8_t *tiles, int tile_value, int colour_bits, const InterLeavesDev &out,
                            hipStream_t s);
// Encoder.  keep (ceil(R.n / 8) bytes), the residual planes res (4 x P.n: r, g, b, tile), the added keys compacted into `added`
// (P.n words) and their number into total_host (pinned, under tag) and cube_added->nfinite.  counts: codec_blocks(P.n) + 1 words.
void inter_match(const InterLeavesDev &R, const InterLeavesDev &P, int colour_bits, uint8_t *keep, uint8_t *res, unsigned long long *added, uint32_t *counts,
                 CodecCube *cube_added, unsigned long long *total_host, uint32_t tag, hipStream_t s);
// the occupancy bytes (zeroed words) of the tree of `n` ascending keys, from codec_count_scan's offsets over a grid for `grid_n` keys
void inter_occupancy(const unsigned long long *keys, uint32_t n, size_t grid_n, int bits, const uint32_t *offsets, const uint64_t depth_offset[16],
                     uint64_t occupancy_bytes, uint32_t *occupancy, hipStream_t s);
// Decoder.  The checks RULE P leaves to the device, after the streams are decoded and A's keys expanded: status (pinned, under tag) =
// 8 an added leaf is a leaf of R | 16 keep's padding bits | 32 kept + added != nleaves.  rank: R.n + 1 words, the kept leaves in
// front of each leaf of R; counts: codec_blocks(R.n) + 1 words; flags: a zeroed word.
void inter_check(const InterLeavesDev &R, const uint8_t *keep, const unsigned long long *added, uint32_t nadded, uint32_t nleaves, uint32_t *rank,
                 uint32_t *counts, uint32_t *flags, unsigned long long *status_host, uint32_t tag, hipStream_t s);
// The frame a checked delta stands for: the merge of the kept and the added keys into P.keys, then per leaf the colours and the tile
// (res: the decoded residual planes, 4 x P.n, the tile plane only with tile_mode 1) into P's planes and the point into dst.
void inter_apply(const InterLeavesDev &R, const uint8_t *keep, const uint32_t *rank, const unsigned long long *added, uint32_t nadded, const uint8_t *res,
                 const CodecDecode &d, int tile_mode, const InterLeavesDev &P, const DeviceSoA &dst, hipStream_t s);

// ---- kernels_lod.hip: level-of-detail decoding (RULE L: hip_ext.h; the arithmetic: lod_terms.hpp) ----
// A frame's leaves as the reduction reads them: the stored colours as RULE C's bit-packed plane (packed != nullptr) or as three byte
// planes of nleaves (RULE P's reference); tiles == nullptr: tile_value throughout.
struct LodSource {
    uint32_t nleaves;
    int colour_bits, tile_value;
    const uint32_t *packed;
    uint64_t colour_words;
    const uint8_t *planes, *tiles;
};
// start[j], j < nruns: the first leaf under node j of depth t, `steps` = b - t lookups in first[] (transform_prepare) below the node's
// number begin + j; start[nruns] = nleaves
void lod_runs_of_tree(const uint32_t *first, uint32_t inner, uint32_t begin, int steps, uint32_t nruns, uint32_t nleaves, uint32_t *start, hipStream_t s);
// The same from n ascending keys of b triples: start (n + 1 words) and the runs' keys of t triples (cut, n words); the number of runs
// goes to total_host (pinned, under tag).  counts: lod_key_runs_words(n) words.
size_t lod_key_runs_words(size_t n);
void lod_runs_of_keys(const unsigned long long *keys, uint32_t n, int b, int t, uint32_t *start, unsigned long long *cut, uint32_t *counts,
                      unsigned long long *total_host, uint32_t tag, hipStream_t s);
// The cloud of L(P, t): the sums of every run (sums: nruns entries, zeroed here), then per new leaf the point of its key (cut, depth
// d.bits = t, d.nleaves = nruns, d.colour_bits as the packet's) with the rounded means and the tiles' OR.
bool lod_points(const LodSource &src, const uint32_t *start, uint32_t nruns, const unsigned long long *cut, CodecLeafSum *sums, const CodecDecode &d,
                const DeviceSoA &dst, hipStream_t s);

}  // namespace k

// Voxel-grid downsample (kernels_voxel.hip).  Returns the new cloud's planes or
// nullptr (error already logged).  leaf_split = positive-cellsize path.
// With `deferred` (octree path only) the call may come back before its kernels are done: it then returns nullptr and
// leaves the pending result in *deferred.
void voxel_sample_streams();   // which of the calling thread's workspace streams are at work: call before the input is resolved (kernels_voxel.hip)
std::shared_ptr<DeviceSoA> voxel_downsample(const std::shared_ptr<DeviceSoA> &src, float cellsize, bool leaf_split, int *error_code,
                                            std::shared_ptr<DeferredResult> *deferred = nullptr);

// Statistical outlier removal (kernels_sor.hip, on the grid of kernels_grid.hip).  Computes d_i into dev_dist
// (n floats, device), returns false on failure.
bool sor_mean_distances(const DeviceSoA &src, int k, float *dev_dist);
// mean/stddev threshold from d_i exactly as pcl::StatisticalOutlierRemoval; result in *thr.
bool sor_threshold(const float *dev_dist, size_t n, float stddev_mul, double *thr);
// The same on the device, nothing read back: *thr_dev (device memory) receives the threshold.
bool sor_threshold_device(const float *dev_dist, size_t n, float stddev_mul, double *thr_dev);
// Stable compaction of points with !(d_i > thr).
std::shared_ptr<DeviceSoA> sor_select(const DeviceSoA &src, const float *dev_dist, double thr, const double *thr_dev = nullptr);
// The outlier filter's last steps on the device: statistics, threshold, compaction.  Small clouds: the statistics' second kernel rides with the compaction's count.
std::shared_ptr<DeviceSoA> sor_threshold_and_select(const DeviceSoA &src, const float *dev_dist, float stddev_mul, double *thr_dev);

// The direction filter's per-point work (kernels_direction.hip): the centroid into centroid_dev (3 device doubles), then per point the
// normal of its neighbourhood (the max_nn nearest within radius), turned away from the centroid.  Each output may be nullptr:
// drop[i] = 0 if normal . dir >= threshold else 1; normals = planes x, y, z of `stride` floats; nn_count[i] = |neighbourhood|.
// No wait inside.  Returns false on failure (logged), also for radius <= 0, a non-finite radius or max_nn outside 1..DIRECTION_MAX_NN.
constexpr int DIRECTION_MAX_NN = 128;
bool direction_normals(const DeviceSoA &src, float radius, int max_nn, const double dir[3], double threshold, float *drop, float *normals,
                       size_t stride, uint32_t *nn_count, double *centroid_dev);

// Euclidean clusters (kernels_cluster.hip; RULE K of hip_ext.h).  One pool block holds everything a call computes, n > 0 points:
//   labels[n], sizes[n] (the first *nclusters are written), nclusters (one word), drop[n] (the keep plane of cluster_keep_flags: 0 keep,
//   1 drop -- what sor_select takes with the threshold 0.5), stats (cluster_labels with with_stats: links seen | unions issued | parent
//   words loaded | most loaded by one union); the rest is the kernels' own.
struct ClusterWork {
    void *block = nullptr;
    size_t n = 0;
    uint32_t *labels = nullptr, *sizes = nullptr;
    const uint32_t *nclusters = nullptr;
    float *drop = nullptr;
    unsigned long long *stats = nullptr;
    uint32_t *parent = nullptr, *root = nullptr, *rootsize = nullptr, *flag = nullptr, *number = nullptr, *state = nullptr;
};
bool cluster_work_alloc(size_t n, ClusterWork &w);   // false: out of memory; the caller gives w.block back to the pool
// labels, sizes and nclusters of src (w.n == src.npoints > 0) for links with d2 < r2.  No wait behind the grid (grid_and_search's sparse
// flow waits inside for the box and the census, as for every search).  False on failure (logged).
bool cluster_labels(const DeviceSoA &src, double r2, bool same_tile, const ClusterWork &w, bool with_stats);
// drop[] from the labels and sizes (RULE K's filter; max_clusters 0: no limit).  No wait.
bool cluster_keep_flags(const ClusterWork &w, uint64_t min_points, uint32_t max_clusters);

// Fixed-radius neighbourhoods (kernels_neigh.hip; RULE N of hip_ext.h), src.npoints > 0.  No wait behind the grid (grid_and_search's
// sparse flow waits inside, as for every search).  False on failure (logged).
// counts[i] (n device words) = |N(i)| - 1, 0 for a point with a non-finite coordinate
bool neigh_counts(const DeviceSoA &src, double r2, bool same_tile, uint32_t *counts);
// drop[i] (n device floats) = 0 (keep) iff point i is finite and counts[i] >= min_neighbours, else 1: what sor_select takes with 0.5
bool neigh_keep_flags(const DeviceSoA &src, const uint32_t *counts, uint64_t min_neighbours, float *drop);
// dst's coordinate planes (dst: src's count and stride) = src smoothed; the CALLER HAS CHECKED the radius (smooth_radius_ok)
bool neigh_smooth(const DeviceSoA &src, double radius, bool same_tile, uint32_t min_neighbours, const DeviceSoA &dst);

// The registration analyzer's search (kernels_nn.hip): per point of `source` the squared f64 distance to its (nth + 1)-th nearest
// point of `reference` among those closer than max_distance (inf: no bound), +inf when there are fewer, into dev_out (source.npoints
// device doubles, the source's order).  No wait inside.  False on failure (logged), also for nth outside 0..NN_MAX_NTH and a
// max_distance that is NaN or <= 0.
constexpr int NN_MAX_NTH = 31;
bool nn_distance2(const DeviceSoA &source, const DeviceSoA &reference, int nth, double max_distance, double *dev_out);
// The same for a table of jobs over one pair of clouds (hip_ext.h: cwipc_hip_nn_job): row j of dev_out (njobs rows of source.npoints
// device doubles) holds job j's squared distances, NaN where the source point takes no part in the job.  dev_table: nn_jobs_table_bytes(njobs)
// bytes of device memory that the caller keeps until it has waited for the stream.  One wait inside (the jobs' participant counts), none
// behind the search.  False on failure (logged), also for njobs outside 1..NN_MAX_JOBS and a job that cwipc_hip_nn_distance2_jobs turns away.
constexpr int NN_MAX_JOBS = 64;
size_t nn_jobs_table_bytes(int njobs);
bool nn_distance2_jobs(const DeviceSoA &source, const DeviceSoA &reference, const cwipc_hip_nn_job *jobs, int njobs, double *dev_out, void *dev_table);
// 1-D Gaussian kernel density estimate (kernels_kde.hip): density[j] = sum_i exp(-0.5 ((at[j] - samples[i]) / h)^2) / (n h sqrt(2 pi)),
// all arrays device memory.  No wait inside.
bool gaussian_kde(const double *dev_samples, size_t n, double h, const double *dev_at, size_t m, double *dev_density);

// ICP fine alignment (kernels_icp.hip; the contracts are at the top of that file).  T, init: 16 f64, row-major 4x4.  All of them wait
// for their results.  False on failure (logged).  THE CALLER HAS CHECKED the scalar arguments (registration.cpp, once for both layers):
// max_distance > 0 (not NaN), a finite matrix, the criteria, radius and max_nn where normals are estimated, epsilon; what depends
// on a cloud's size is checked here: false also for a caller's normal that is not finite.
struct IcpCriteria { double relative_fitness, relative_rmse; int max_iteration; };   // open3d's ICPConvergenceCriteria
// An aligner's answer.  The caller sets T to the initial matrix and the rest to 0; an aligner that has nothing to do (an empty
// cloud) or fails leaves it so.
struct IcpResult { double T[16]; double fitness, inlier_rmse; int iterations; };
// Per source point the original index of its nearest reference point and the squared distance (0xFFFFFFFF / +inf: none) into host arrays, either may be nullptr.
bool icp_correspondences(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, uint32_t *idx_host,
                         double *d2_host);
// One search and the fit sums over its matches: sums = sum a (3) | sum b (3) | sum a b^T (9) | sum d2, a = T p - cp, b = q - cq.
// False also for a pivot that is not finite.
bool icp_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, const double cp[3], const double cq[3],
              uint64_t *n, double sums[16]);
// open3d's registration_icp with the point-to-point estimate; cp0, cq: the clouds' centroids (the pivots: T cp0 and cq).
bool icp_point2point(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const IcpCriteria &k, const double cp0[3],
                     const double cq[3], IcpResult &res);
// Point-to-plane ICP.  host_normals: the reference cloud's normals as three planes of reference.npoints floats (x, y, z) in host
// memory, or nullptr: direction_normals(radius, max_nn) estimates them on the device.
// sums = sum J J^T (21, upper triangle row-major) | sum J r (6) | sum r^2 | sum d2.
bool icp_plane_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, const float *host_normals, float radius,
                    int max_nn, uint64_t *n, double sums[29]);
// open3d's registration_icp with the point-to-plane estimate (plane_fit.hpp).
bool icp_point2plane(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const float *host_normals, float radius, int max_nn,
                     const IcpCriteria &k, IcpResult &res);
// Generalized ICP (gicp_terms.hpp).  Both clouds have normals, each array as for point-to-plane (host planes, or nullptr: estimated
// on the device); they are turned as the reference's _fix_normal_direction turns them and give each point a covariance.
// The parity entry: per point of `cloud` the six values 00, 01, 02, 11, 12, 22 into cov_host (cloud.npoints rows of 6 doubles);
// direction nullptr: the normals are not turned.
bool icp_gicp_covariances(const DeviceSoA &cloud, const float *host_normals, float radius, int max_nn, const double *direction, double epsilon,
                          double *cov_host);
// sums = sum (A^T N A)_ij for i <= j (21) | sum (A^T g)_i (6) | sum e^T g | sum d2: the plane sums' layout.
bool icp_gicp_sums(const DeviceSoA &source, const DeviceSoA &reference, const double T[16], double max_distance, const float *source_normals,
                   const float *reference_normals, float radius, int max_nn, double epsilon, uint64_t *n, double sums[29]);
// open3d's registration_generalized_icp: the same loop with these sums and the point-to-plane update.
bool icp_generalized(const DeviceSoA &source, const DeviceSoA &reference, double max_distance, const float *source_normals,
                     const float *reference_normals, float radius, int max_nn, double epsilon, const IcpCriteria &k, IcpResult &res);
// RULE Q (hip_ext.h; the terms are quality_terms.hpp): the distortion sums of `degraded` against `original`, out[0] forward (source
// the original), out[1] backward.  host_normals: the ORIGINAL's, as for point-to-plane; plane false: no normals are made or read.
// Two passes of grid, search and sums, one wait each.  The caller has also checked that host_normals are finite (before either cloud
// is brought to the device: a refused call launches and allocates nothing).
bool icp_distortion(const DeviceSoA &original, const DeviceSoA &degraded, double max_distance, const float *host_normals, float radius, int max_nn,
                    bool plane, cwipc_hip_distortion_sums out[2]);
// the mean of a cloud's points (the direction filter's centroid kernels) on the host; non-finite where a coordinate is
bool icp_centroid(const DeviceSoA &cloud, double cen[3]);

// Generic stable compaction driver used by tilefilter / crop / masked filter.
// may_return_early: the call may come back with the scatter kernel still running (the result carries a
// `ready` event); only for predicates that refer to nothing the caller frees afterwards.
std::shared_ptr<DeviceSoA> compact(const DeviceSoA &src, const k::Predicate &p, bool may_return_early = false);

}  // namespace cwipc_amd
