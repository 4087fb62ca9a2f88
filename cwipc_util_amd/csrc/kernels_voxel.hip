// kernels_voxel.hip -- voxel-grid downsample on gfx950 (MI355X).
//
// Reference: cwipc_downsample / cwipc_downsample_voxelgrid, src/cwipc_filters.cpp:30-172.
// The arithmetic the reference delegates to PCL is restated from the published
// upstream algorithms (scalar restatement: oracle/cwipc_oracle.c):
//   pcl::VoxelGrid            voxel (i,j,k) = floor(p * (1/leaf)) with an fp32 product; one
//                             output per occupied voxel = mean xyz, truncated mean rgb;
//                             outputs in ascending (k,j,i); grids above 2^31 cells refused.
//   pcl::octree::OctreePointCloud (positive cellsize only) leaves of side R = 64*leaf on a
//                             lattice anchored at the first point; every leaf is voxelised on
//                             its own, so a voxel cut by a leaf face yields one output per
//                             side; leaves are emitted in depth-first (Morton) order of their
//                             final octree keys, which depend on how the bounding box grew
//                             while the points were inserted in input order.
//   tile of an output         OR of the tiles of its contributors (src/cwipc_filters.cpp:64-74).
//
// Design for MI355X.  The job is HBM-bound integer work: 16 B per input point must be read
// once (160 MB at the 10 M-point configuration, ~29.5 us at the 5.4 TB/s a pure read of these
// planes reaches on this part), everything else has to hide behind that stream.  Measured
// constraints that shaped the kernel (scratch/ubench*.hip):
//   * scattered global integer atomics retire at ~23 G requests/s chip-wide whatever their
//     scope, but 8 lanes updating one 64-byte record cost ~1.3 requests (17 G records/s);
//   * many lanes bumping ONE counter serialise at the memory side (40 k of them: ~250 us);
//   * an LDS atomic costs 13-20 cycles per WAVE INSTRUCTION almost independent of the
//     number of active lanes, so instructions have to be saved, not lanes;
//   * f64 and out-of-line calls in the streaming loop cost more than the stream itself.
// Hence:
//   host                  the octree lattice is anchored at the cloud's first point, which the
//                         host knows (or fetches once): it computes the anchor and, per axis, a
//                         table of leaf-face thresholds with the octree's own f64 arithmetic
//                         (the octree key floor((p - min)/res) is monotone in p, so "key >= m"
//                         is exactly "p >= T(m)" for one float T(m)).
//   K1 voxel_accumulate   persistent: one 1024-lane workgroup per CU, every wave streams a
//                         contiguous range of the planes (dwordx4 per plane per lane, next
//                         step prefetched in registers).  fp32/integer only.  Two variants with
//                         identical integer sums: the fast one (voxel_k1_fast.inc: linear voxel
//                         keys, leaf side bits from per-wave slabs, wave-wide prefix sums, one
//                         conflict-free LDS insert per run) takes clouds in scan order; the general
//                         one (voxel_k1_general.inc: leaf by threshold compare, DPP segmented scan over chains of
//                         lanes, overflow path to the global records) takes everything else and is
//                         what the fast one hands a cloud back to (ERR_FAST_PATH).  Either way the
//                         workgroup's LDS table is flushed ONCE into dense per-leaf grids of
//                         64-byte records, 8 lanes per record; first touches (told by the returned
//                         count, in the fast variant by the leaf's occupancy bit) are counted per
//                         bitmap slice.  All sums are
//                         integers: results are bitwise reproducible.  Each wave also emits the
//                         bounding box of its range.
//   (partition)           clouds in no spatial order first go through voxel_partition.inc: bucket
//                         histogram + range boxes of the original order, scan, LDS-staged scatter;
//                         K1 (general) then runs on the moved copy.
//   K2 octree_replay      one workgroup replays the octree's bounding-box growth over the wave
//                         boxes, re-reading only the ranges that trigger a growth step
//                         (plain grid: reduces the boxes to the global one); publishes the pass's
//                         control words to pinned host memory.
//   rank_emit             octree path: output position = rank of the cell's bit in the occupancy
//                         bitmaps (leaves in Morton order of their final keys), centroid / colour /
//                         tile from the record, record and bit zeroed for the next call.  Launched
//                         right behind K2, before the host knows the count; a stream of frames gets
//                         its results back while these kernels run (PendingVoxel).
//   grid_mark .. unmark   plain grid: the same through a bitmap over the VoxelGrid index space.
//   make_sort_keys + rocprim radix sort + emit_and_clean: only for plain-grid index spaces beyond
//                         2^28 cells.
// Parts of this translation unit: voxel_common.hpp (constants, error bits, control words, parameter blocks, leaf table and record helpers),
// voxel_anchor.hpp (host arithmetic without a HIP type: anchor box, face thresholds, range plans; host-tested), voxel_k1_general.inc,
// voxel_k1_fast.inc, voxel_partition.inc, voxel_finalize.inc (replay, finalize, clean-up kernels); this file: the workspace, a pass's
// report and voxel_downsample() as a sequence of steps (VoxCall).
#include "internal.hpp"

#include <atomic>
#include <chrono>

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include <cfloat>
#include <type_traits>
#include <cmath>

#include "voxel_anchor.hpp"
#include "voxel_common.hpp"

namespace cwipc_amd {

namespace {

#include "voxel_k1_general.inc"
#include "voxel_k1_fast.inc"
#include "voxel_partition.inc"
#include "voxel_finalize.inc"

// ---------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------
// An octree pass whose call has returned (DeferredResult): accumulate, replay and finalize kernels are in flight, the
// finalize kernel writes into `spec_dst`, sized from the passes before.  Whoever needs the outcome polls the workspace's
// pinned words for this pass's sequence number.  If the pass did not go through (an error word, more outputs than
// spec_dst holds) the result is computed again by an ordinary, waiting call, and the workspace's next user cleans up.
struct PendingVoxel : DeferredResult {
    std::recursive_mutex lock;   // (settle() may run the pass again on this thread, which first asks the workspace's pending pass -- this one -- for its outcome)
    std::shared_ptr<DeviceSoA> src, spec_dst, result;
    volatile unsigned long long *words = nullptr;
    hipStream_t stream = nullptr;
    uint32_t seq = 0, spec_cap = 0;
    float cellsize = 0;
    bool known = false, ok = false, settled = false;
    uint32_t err = 0, m = 0;
    bool leaf_split = true;                      // octree pass; false: the plain grid, whose finalize kernels ran only if the index space fits (gspec)
    GridSpec gspec{0, 0u, 0u, 0ull};
    bool partitioned = false;                    // the pass ran on a partitioned copy of the cloud ...
    uint32_t scatter = 0, steps_total = 0;       //   ... and this is how scattered the cloud was as it came (of how many wave steps)
    uint32_t leaves = 0;                         // leaf grids the pass used
    bool outcome_locked();                       // waits for the replay kernel's report; true: spec_dst holds the result
    bool outcome() { std::lock_guard<std::recursive_mutex> g(lock); return outcome_locked(); }
    std::shared_ptr<DeviceSoA> settle() override;
};

std::atomic<size_t> g_workspace_bytes{0};   // device memory held by voxel workspaces (cwipc_hip_workspace_bytes)
constexpr size_t GRID_BYTES = (size_t)CELLS * RECORD_WORDS * 8;   // 20.1 MB per leaf grid
constexpr size_t HEAD_CTRL_BYTES = 256;                           // C_WORDS words, padded

struct Workspace {
    int device = -1;
    size_t grid_bytes = 0;             // what this workspace has added to g_workspace_bytes
    int cus = 0, cus_device = -1;   // compute units of the device the workspace was last used on
    uint32_t leaf_cap = 0;     // leaf hash capacity = number of grids (power of two)
    size_t list_cap = 0;
    size_t bbox_cap = 0;
    void *head = nullptr;              // two blocks of ctrl | leaf_keys | seg_count, used by alternate passes
    size_t head_bytes = 0;             // bytes of one block
    int parity = 0;                    // block of the next pass
    uint32_t seq = 0;                  // sequence number of the last pass (never 0 once used)
    uint32_t last_m = 0;               // outputs of this thread's last octree pass (sizes the speculative result of the next)
    uint32_t last_m_grid = 0;          //   ... and of its last plain-grid pass
    int shrink = 0;                    // log2 of how much smaller than "one workgroup per CU" the workgroups are made (sparse clouds)
    int calm = 0;                      // calls in a row whose tables stayed less than a third full
    bool incoherent = false;           // smaller workgroups did not stop the overflows: stay with full-size ones
    bool no_fast = false;              // the fast accumulate kernel gave this kind of cloud back (ERR_FAST_PATH): use the general one
    int streak = 0;                    // octree passes of this kind in a row that went through without a retry
    int roomy = 0;                     // passes in a row that used at most a quarter of the leaf grids
    uint32_t shrink_to = 0;            // != 0: give the grids back and start again with this many (at the next call, when nothing is in flight)
    // A leaf grid is 20 MB: a thread that once met a cloud of many leaves must not sit on them while it filters camera tiles
    // of three or four.  Eight roomy passes in a row -> the next call reallocates for what these passes needed.
    void note_leaves(uint32_t leaves) {
        uint32_t need = 4;
        while (need < leaves) need <<= 1;
        if (need * 4 <= leaf_cap) {
            if (++roomy >= 8) shrink_to = need;
        } else {
            roomy = 0;
            shrink_to = 0;
        }
    }
    uint32_t *host_words = nullptr;    // page-locked: the replay kernel publishes the pass's control words here (64-bit, tagged with seq)
    std::shared_ptr<struct PendingVoxel> pending;   // the pass still in flight on this workspace, if the call that started it has returned
    size_t hint_n = 0;                 // the kind of call ws.shrink was learned on
    float hint_cell = 0.f;
    bool hint_split = true;
    bool head_clean[2] = {false, false};   // the block is known to be zero (the replay kernel of the pass before zeroed it)
    unsigned long long *leaf_keys = nullptr;
    unsigned long long *hash_keys = nullptr;
    uint32_t *hash_ids = nullptr;
    unsigned long long *records = nullptr;
    uint32_t *occupied = nullptr;
    uint32_t *order = nullptr;         // records in output order (finalize pass), list_cap entries
    uint32_t *gbits = nullptr;         // plain grid: bitmap over the VoxelGrid index space, its per-word and per-block prefixes
    uint32_t *gprefix = nullptr, *gblock = nullptr;
    size_t gwords_cap = 0;
    float *bboxes = nullptr;           // [2][bbox_cap][6]: the ranges' boxes the replay kernel reads; behind them room for boxes nobody reads
    float *part = nullptr;             // partition pass: the cloud moved into spatial buckets, four planes of part_stride elements
    size_t part_stride = 0;
    uint32_t *part_hist = nullptr;     //   ... and its table: a row of PART_BUCKETS counts per range, the rows' sums by segments, the buckets' starts
    size_t part_rows = 0;              //   (room for this many rows)
    uint32_t *ctrl = nullptr;
    uint32_t *bitmaps = nullptr;
    uint32_t *seg_count = nullptr;
    float *faces = nullptr;            // device copy of the threshold table
    uint32_t faces_host[FACE_TABLE_WORDS];   // what the device copy holds
    double faces_mn0[3] = {0, 0, 0};   //   ... and what it was computed from
    double faces_res = 0;
    bool faces_valid = false;
    void drop_partition_buffers() {
        if (part) { (void)hipFree(part); g_workspace_bytes -= 16 * part_stride; }
        if (part_hist) (void)hipFree(part_hist);
        part = nullptr; part_hist = nullptr; part_stride = 0; part_rows = 0;
    }
    VoxWork work() const { return VoxWork{leaf_keys, records, occupied, ctrl, bboxes, faces, bitmaps, seg_count, hash_keys, hash_ids}; }
    // control words, leaf table, slice counts, leaf hash: a pass works on one of the two blocks
    char *bind_head(int blk) {
        char *h = (char *)head + (size_t)blk * head_bytes;
        ctrl = (uint32_t *)h;
        leaf_keys = (unsigned long long *)(h + HEAD_CTRL_BYTES);
        seg_count = (uint32_t *)(h + HEAD_CTRL_BYTES + (size_t)leaf_cap * 8);
        hash_keys = (unsigned long long *)(h + HEAD_CTRL_BYTES + (size_t)leaf_cap * 8 + (size_t)leaf_cap * RANK_SEGS * sizeof(uint32_t));
        hash_ids = (uint32_t *)((char *)hash_keys + (size_t)leaf_cap * 4 * 8);
        return h;
    }
    // the leaf grids (head blocks, records, occupancy bitmaps) go back to the device; errors ignored (release())
    void free_grids() {
        if (head) (void)hipFree(head);
        if (records) (void)hipFree(records);
        if (bitmaps) (void)hipFree(bitmaps);
        head = nullptr; ctrl = nullptr; leaf_keys = nullptr; seg_count = nullptr; records = nullptr; bitmaps = nullptr;
        g_workspace_bytes -= grid_bytes;
        grid_bytes = 0;
        leaf_cap = 0;
    }
    void free_index_bitmap() {
        if (gbits) (void)hipFree(gbits);
        if (gprefix) (void)hipFree(gprefix);
        if (gblock) (void)hipFree(gblock);
        gbits = gprefix = gblock = nullptr; gwords_cap = 0;
    }
    void release() {
        // also runs at thread exit, when the runtime may be gone: errors ignored
        free_grids();
        head_bytes = 0;
        if (occupied) (void)hipFree(occupied);
        if (order) (void)hipFree(order);
        free_index_bitmap();
        if (bboxes) (void)hipFree(bboxes);
        drop_partition_buffers();
        if (faces) (void)hipFree(faces);
        if (host_words) (void)hipHostFree(host_words);
        host_words = nullptr;
        occupied = nullptr; order = nullptr; bboxes = nullptr; faces = nullptr;
        list_cap = 0; bbox_cap = 0;
        faces_valid = false;
    }
    ~Workspace() { release(); }
};

// Two workspaces per thread, used by alternate calls, each with its own stream (ThreadCtx::stream / stream_alt):
// a call's finalize kernel, still running when the call returns, works on grids the next call does not touch.
// The workspaces of threads that have ended wait here for the next thread (1.3 GB each: a program that starts a
// thread per frame must not allocate and free that much every time).
std::mutex g_ws_pool_mutex;
std::vector<Workspace *> *g_ws_pool = new std::vector<Workspace *>();   // never destroyed: threads may end after the statics

constexpr int MAX_WS = 2 + ThreadCtx::EXTRA_STREAMS;   // workspaces (and streams) a thread's calls rotate over, at most
struct WorkspaceLease {
    Workspace *ws[MAX_WS] = {nullptr, nullptr, nullptr, nullptr};
    Workspace &get(int which) {
        if (!ws[which]) {
            const int dev = current_device();
            std::lock_guard<std::mutex> lock(g_ws_pool_mutex);
            for (size_t i = 0; i < g_ws_pool->size(); i++) {
                if ((*g_ws_pool)[i]->device == dev) {   // one that already holds grids on this device
                    ws[which] = (*g_ws_pool)[i];
                    g_ws_pool->erase(g_ws_pool->begin() + (long)i);
                    break;
                }
            }
            if (!ws[which]) ws[which] = new Workspace();
        }
        return *ws[which];
    }
    ~WorkspaceLease() {
        // thread exit: a finalize kernel of this thread's last call may still be using a workspace
        bool any = false;
        for (int i = 0; i < MAX_WS; i++) any = any || ws[i];
        if (any) (void)hipDeviceSynchronize();
        // A pass of this thread that was handed out while it ran (ws.pending) reads its report from the workspace's pinned words
        // when somebody asks for the result -- possibly another thread, long after this one has gone and the workspace with
        // it.  The report is final now: take it (the outcome is cached in the pending pass, the words are not looked at again).
        // A workspace that goes to the pool keeps its `pending`: its next user learns from it whether the records were left clean.
        for (int i = 0; i < MAX_WS; i++)
            if (ws[i] && ws[i]->pending) (void)ws[i]->pending->outcome();
        // (r3: at most eight wait here -- a program with a thread per tile and frame finds one each; what threads held beyond
        // that, mostly second workspaces that a busy moment made them take, is given back to the device)
        std::vector<Workspace *> surplus;
        {
            std::lock_guard<std::mutex> lock(g_ws_pool_mutex);
            for (int i = 0; i < MAX_WS; i++) {
                if (!ws[i]) continue;
                if (g_ws_pool->size() < 8) g_ws_pool->push_back(ws[i]);
                else surplus.push_back(ws[i]);
            }
        }
        for (Workspace *w : surplus) delete w;
    }
};
thread_local WorkspaceLease t_ws;
thread_local int t_ws_next = 0;
thread_local uint32_t t_busy_sample = 0;    // bit i: the stream of this thread's workspace i had work in flight when cwipc_downsample was entered
thread_local bool t_busy_sampled = false;  // ... valid for the call that follows (voxel_sample_streams)
thread_local int t_ws_idle = 0;   // calls in a row that found both of the thread's streams idle while it holds a second workspace

// The stream of a thread's workspace i (the extra ones are created on first use; nullptr where that failed).
hipStream_t &workspace_stream(ThreadCtx &c, int i) {
    if (i >= 2) (void)c.extra_stream(i - 2);
    return i == 0 ? c.stream : i == 1 ? c.stream_alt : c.stream_extra[i - 2];
}

// For the duration of a call: the thread's current stream is the one of the workspace in use.
struct StreamOfWorkspace {
    ThreadCtx &c;
    hipStream_t *other = nullptr;   // the stream that changed places with c.stream for the duration of the call
    StreamOfWorkspace(ThreadCtx &ctx, int which) : c(ctx) {
        if (which > 0 && workspace_stream(c, which)) other = &workspace_stream(c, which);
        if (other) std::swap(c.stream, *other);
    }
    ~StreamOfWorkspace() {
        if (other) std::swap(c.stream, *other);
    }
};

bool ensure_workspace(Workspace &ws, size_t n, uint32_t leaf_cap, uint32_t nranges, hipStream_t s) {
    const int dev = current_device();
    if (ws.device != dev) {
        ws.release();
        const int lds = (int)sizeof(LdsTable);
        CW_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&voxel_accumulate_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        CW_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&voxel_accumulate_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        CW_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&voxel_accumulate_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        const int lds_fast = (int)sizeof(FastTable);
        CW_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&voxel_accumulate_fast_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_fast));
        CW_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&voxel_accumulate_fast_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_fast));
        CW_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&partition_scatter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PartLds)));
        ws.device = dev;
    }
    if (ws.leaf_cap < leaf_cap) {
        ws.free_grids();
        ws.head_bytes = HEAD_CTRL_BYTES + (size_t)leaf_cap * 8 + (size_t)leaf_cap * RANK_SEGS * sizeof(uint32_t) + (size_t)leaf_cap * 4 * (8 + 4);
        ws.head_bytes = (ws.head_bytes + 255) & ~(size_t)255;
        CW_HIP_TRY(hipMalloc(&ws.head, 2 * ws.head_bytes));
        ws.head_clean[0] = ws.head_clean[1] = false;
        ws.parity = 0;
        CW_HIP_TRY(hipMalloc((void **)&ws.bitmaps, (size_t)leaf_cap * BITWORDS * sizeof(uint32_t)));
        CW_HIP_TRY(hipMemsetAsync(ws.bitmaps, 0, (size_t)leaf_cap * BITWORDS * sizeof(uint32_t), s));
        CW_HIP_TRY(hipMalloc((void **)&ws.records, (size_t)leaf_cap * GRID_BYTES));
        CW_HIP_TRY(hipMemsetAsync(ws.records, 0, (size_t)leaf_cap * GRID_BYTES, s));   // once; K4 keeps it clean afterwards
        ws.leaf_cap = leaf_cap;
        ws.grid_bytes = (size_t)leaf_cap * (GRID_BYTES + BITWORDS * sizeof(uint32_t)) + 2 * ws.head_bytes;
        g_workspace_bytes += ws.grid_bytes;
    }
    if (ws.list_cap < n) {
        if (ws.occupied) (void)hipFree(ws.occupied);
        if (ws.order) (void)hipFree(ws.order);
        ws.occupied = nullptr; ws.order = nullptr; ws.list_cap = 0;
        CW_HIP_TRY(hipMalloc((void **)&ws.occupied, n * sizeof(uint32_t)));
        CW_HIP_TRY(hipMalloc((void **)&ws.order, n * sizeof(uint32_t)));
        ws.list_cap = n;
    }
    if (ws.bbox_cap < nranges) {
        if (ws.bboxes) (void)hipFree(ws.bboxes);
        ws.bboxes = nullptr; ws.bbox_cap = 0;
        CW_HIP_TRY(hipMalloc((void **)&ws.bboxes, 2 * (size_t)nranges * 6 * sizeof(float)));
        ws.bbox_cap = nranges;
    }
    if (!ws.faces) CW_HIP_TRY(hipMalloc((void **)&ws.faces, FACE_TABLE_WORDS * sizeof(uint32_t)));
    if (!ws.host_words) {
        CW_HIP_TRY(hipHostMalloc((void **)&ws.host_words, 2 * C_WORDS * sizeof(uint32_t), hipHostMallocDefault));
        memset(ws.host_words, 0, 2 * C_WORDS * sizeof(uint32_t));
    }
    return true;
}

bool fetch_first_point(const DeviceSoA &src, ThreadCtx &c) {
    if (src.has_first) return true;
    float *h = (float *)c.host_words;
    hipLaunchKernelGGL(first_point_kernel, dim3(1), dim3(1), 0, c.stream, src.x(), src.y(), src.z(), h);
    bool ok = hipGetLastError() == hipSuccess;
    ok = c.sync() && ok;
    if (!ok) return hip_failed(hipGetLastError(), "fetch of the first point", __FILE__, __LINE__);
    src.first[0] = h[0]; src.first[1] = h[1]; src.first[2] = h[2];
    src.has_first = true;
    return true;
}

// A pass's report: the control words the replay kernel published into the workspace's pinned words, tagged with the pass's number.
struct PassReport {
    uint32_t w[C_SEQ];
    bool seen = false;   // every word carried this pass's tag
    uint32_t operator[](int i) const { return w[i]; }
};

// Reads it: polls the pinned words while `poll` (for the poll budget at most: a few hundred microseconds as a rule; a blocking
// stream wait wakes up several microseconds late), then `stream_wait()`, the caller's way of waiting for the stream, and where that
// returns true one more look.
template <class StreamWait>
PassReport read_report(volatile unsigned long long *words, uint32_t seq, bool poll, const StreamWait &stream_wait) {
    PassReport r;
    const auto take = [&]() {   // true when every word carries this pass's tag
        for (int i = 0; i < C_SEQ; i++) {
            const unsigned long long w = words[i];
            if ((uint32_t)(w >> 32) != seq) return false;
            r.w[i] = (uint32_t)w;
        }
        return true;
    };
    if (poll) {
        const auto t_give_up = std::chrono::steady_clock::now() + std::chrono::microseconds(poll_budget_us());
        for (int spin = 0;; spin++) {
            if ((uint32_t)(words[C_COUNT] >> 32) == seq && take()) { r.seen = true; break; }
            if ((spin & 255) == 255 && std::chrono::steady_clock::now() > t_give_up) break;
            __builtin_ia32_pause();
        }
    }
    if (!r.seen && stream_wait()) r.seen = take();
    std::atomic_thread_fence(std::memory_order_acquire);
    return r;
}

// Did the speculative grid passes run?  (the test grid_gate made on the device, on the same words, for a pass without an error)
bool grid_fits(const PassReport &hw, const GridSpec &spec) {
    const unsigned long long cells = (unsigned long long)hw[C_DIVB] * hw[C_DIVB + 1] * hw[C_DIVB + 2];
    return hw[C_COUNT] <= spec.m_cap && cells <= spec.cells_max && (cells + 31) / 32 <= spec.words_cap;
}

// A pass without an output (only points that do not count, non-finite ones): the reference's VoxelGrid path reports an empty
// result (reference src/cwipc_filters.cpp:58-62), the octree has no leaves and gives an empty cloud.
std::shared_ptr<DeviceSoA> empty_result(bool leaf_split) {
    if (leaf_split) return soa_alloc(0);
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_downsample", "VoxelGrid filter produced empty pointcloud");
    return nullptr;
}

// What a finished pass teaches the workspace whichever call reads its report, the one that started it or the next one on the
// workspace: the count that sizes the next speculative result (none after a pass that did not go through), and, from a partitioned
// pass, how scattered the cloud was as it came: in scan order again -> no partition next time.
void learn_from_pass(Workspace &ws, bool leaf_split, bool went_through, uint32_t m, bool partitioned, uint32_t scatter, size_t steps_total) {
    (leaf_split ? ws.last_m : ws.last_m_grid) = went_through ? m : 0;
    if (partitioned && (size_t)scatter * 4 < steps_total) ws.incoherent = false;
}

bool PendingVoxel::outcome_locked() {
    if (known) return ok;
    const PassReport hw = read_report(words, seq, true, [&]() {
        if (hipStreamSynchronize(stream) != hipSuccess) (void)hipGetLastError();
        return true;
    });
    known = true;
    err = hw.seen ? hw[C_ERR] : 0x80000000u;
    m = hw.seen ? hw[C_COUNT] : 0u;
    scatter = hw.seen ? hw[C_SCATTER] : 0xffffffffu;
    leaves = hw.seen ? hw[C_LEAVES] : 0u;
    ok = hw.seen && err == 0u && m <= spec_cap;
    if (ok && !leaf_split) ok = grid_fits(hw, gspec);
    return ok;
}

std::shared_ptr<DeviceSoA> PendingVoxel::settle() {
    std::lock_guard<std::recursive_mutex> g(lock);
    if (settled) return result;
    if (outcome_locked()) {
        if (m == 0) {
            result = empty_result(leaf_split);
        } else {
            spec_dst->npoints = m;   // the finalize kernel is filling (or has filled) the first m slots; the planes carry its `ready` event
            result = spec_dst;
        }
    } else {
        // not a pass that could be handed out early after all: once more, the waiting way (the dirty records of the
        // failed pass are cleaned by the next user of its workspace)
        int code = 0;
        result = voxel_downsample(src, cellsize, leaf_split, &code, nullptr);
    }
    spec_dst.reset();
    src.reset();
    settled = true;
    return result;
}

// One call of voxel_downsample(): its state, and its steps in the order the driver takes them.
struct VoxCall {
    ThreadCtx &c;
    Workspace &ws;
    const std::shared_ptr<DeviceSoA> &src_ptr;
    const DeviceSoA &src;
    const float cellsize;
    const bool leaf_split;
    const size_t n;
    // the plan
    int cus = 0;
    size_t steps_total = 0, nwaves = 0, part_nseg = 0;
    uint32_t nblocks = 0, faces_host[FACE_TABLE_WORDS];
    double faces_key_mn0[3] = {0, 0, 0};
    bool partition = false;
    VoxParams P;
    // what a retry changes: grids, the accumulate kernel's mode (0 plain grid, 1 octree by face thresholds, 2 octree by f64 division),
    // and whether leaf ids are resolved per workgroup at flush time (off after ERR_LOCAL_LEAVES)
    uint32_t leaf_cap = 0;
    int mode;
    bool local_leaves = true;
    // the pass in hand (ok: no runtime call of the pass has failed)
    bool ok = true, used_fast = false;
    hipError_t launch_err = hipSuccess;
    uint32_t seq = 0, err = 0, spec_cap = 0;
    VoxWork W;
    char *next_head = nullptr;
    FastPlan fplan{0u, 0u, 0u, 0u};
    std::shared_ptr<DeviceSoA> spec_dst;
    GridSpec gspec{0, 0u, 0u, 0ull};
    unsigned long long bitmap_max = GRID_BITMAP_MAX_CELLS;
    VoxCall(ThreadCtx &ctx, Workspace &w, const std::shared_ptr<DeviceSoA> &s, float cell, bool split)
        : c(ctx), ws(w), src_ptr(s), src(*s), cellsize(cell), leaf_split(split), n(s->npoints), mode(split ? 1 : 0) {}

    // the steps, in the order voxel_downsample() takes them
    bool collect_pending(); void plan(); bool anchor_and_faces(std::shared_ptr<DeviceSoA> &early); bool partition_buffers(); bool first_leaf_cap();
    bool setup_pass(); void launch_accumulate(); void launch_replay(); void launch_speculative();
    void launch_grid_finalize(const GridSpec &spec, uint32_t count, uint32_t words, DeviceSoA &dst);
    bool hand_out(int attempt, std::shared_ptr<DeferredResult> *deferred); PassReport await_report(); void adapt_workgroups(const PassReport &hw);
    std::shared_ptr<DeviceSoA> finalize(const PassReport &hw, uint32_t m);
    bool retry_or_report(int attempt, const PassReport &hw, uint32_t m, std::shared_ptr<DeviceSoA> &dst);
};

// Which of the thread's workspaces takes this call.
int pick_workspace(ThreadCtx &c) {
    // Workspaces (and streams) per thread, taken in turn, so that a call queued right behind another does not wait for that one's
    // finalize kernel.  The second one comes into being only when it is needed: a thread whose downsample calls are separated by
    // other work (a per-tile filter chain) finds its first workspace idle every time and never pays the 80+ MB of grids for a second.
    // r4: and a third (CWIPC_WORKSPACES, 1 to 4, default 3) when the one whose turn it is still has kernels in flight: the kernel
    // trace of a stream of calls (gpurun_out/r4_trace_dump.log) shows a call's chain on its stream -- accumulate 54-65 us next to its
    // neighbour, replay 7, finalize 16-27, and the host's turn-around -- at ~110 us, i.e. two streams give a call every 55 us whatever
    // the accumulate kernel does; the chip had nothing to stream for 12 of every 110 us.
    static const int max_ws = []() { const char *e = getenv("CWIPC_WORKSPACES"); const int v = e ? atoi(e) : 3; return v < 1 ? 1 : v > MAX_WS ? MAX_WS : v; }();
    int have = 0;
    while (have < MAX_WS && t_ws.ws[have]) have++;
    const bool sampled = t_busy_sampled;
    t_busy_sampled = false;
    const auto busy = [&](int i) {
        if (sampled) return ((t_busy_sample >> i) & 1u) != 0u;   // as the thread's streams were when the call came in (voxel_sample_streams)
        hipStream_t s = workspace_stream(c, i);
        const bool b = s && hipStreamQuery(s) == hipErrorNotReady;
        (void)hipGetLastError();   // (hipErrorNotReady is an answer, not a failure)
        return b;
    };
    int which = 0;
    if (have > 0) {
        which = t_ws_next % have;
        if (have < max_ws && busy(which)) {
            which = have;          // this thread's calls come faster than its workspaces turn around: one more
        } else if (have > 1 && !t_ws.ws[have - 1]->pending) {
            // ... and the last one goes again when it has not been needed for a while: sixteen calls in a row that found all streams idle (a
            // thread that has stopped calling back to back: 0.3 GB of leaf grids it no longer needs)
            bool idle = true;
            for (int i = 0; i < have && idle; i++) idle = !busy(i);
            t_ws_idle = idle ? t_ws_idle + 1 : 0;
            if (t_ws_idle >= 16) {
                delete t_ws.ws[have - 1];
                t_ws.ws[have - 1] = nullptr;
                have--;
                t_ws_idle = 0;
                which = which % have;
            }
        }
    }
    t_ws_next = which + 1;
    return which;
}

// The pass before last of this thread on the workspace, if it was handed out while it ran.
bool VoxCall::collect_pending() {
    if (!ws.pending) return true;
    // the pass before last of this thread was handed out while it ran: its report is in by now (its words are about to
    // be reused); if it did not go through, its records are still dirty
    const std::shared_ptr<PendingVoxel> p = ws.pending;
    ws.pending.reset();
    const bool went_through = p->outcome();
    learn_from_pass(ws, p->leaf_split, went_through, p->m, went_through && p->partitioned, p->scatter, p->steps_total);
    if (went_through) {
        ws.note_leaves(p->leaves);
        return true;
    }
    ws.streak = 0;
    if (p->err & (ERR_FAST_PATH | ERR_CELL_RANGE)) ws.no_fast = true;
    CW_LAUNCH("clean_by_bitmap", clean_by_bitmap_kernel, dim3(ws.leaf_cap * RANK_SEGS), dim3(RANK_THREADS), 0, c.stream, ws.work());
    if (!c.sync()) { hip_failed(hipGetLastError(), "voxel workspace clean-up", __FILE__, __LINE__); return false; }
    return true;
}

// CUs, wave ranges and the parameter block.
void VoxCall::plan() {
    // (asked once per workspace and device: a runtime call on the way to the first launch is time the GPU waits)
    if (ws.cus_device != current_device() || ws.cus <= 0) {
        int cus_now = 0;
        if (hipDeviceGetAttribute(&cus_now, hipDeviceAttributeMultiprocessorCount, current_device()) != hipSuccess || cus_now <= 0) cus_now = 256;
        ws.cus = cus_now;
        ws.cus_device = current_device();
    }
    // The persistent grid leaves one compute unit per XCD free (8 of 256 on MI355X).  In a stream of calls consecutive
    // accumulate kernels run on the thread's two streams: the next one's workgroups start on the free CUs and take over the
    // others as the previous kernel's workgroups finish, so one kernel's start-up and flush (about 10 of its 58 us, during
    // which a CU streams nothing) lie behind the other's stream: 61.3 -> 52.5 us per call at 10 M points.  It takes a free CU
    // on EVERY XCD (workgroups are dealt to the XCDs in turn: with 6 spare CUs nothing is gained, with 8 everything); a
    // single kernel is as fast on 248 CUs as on 256 (58.8 / 58.5 us).  CWIPC_SPARE_CUS=n overrides (a process that runs a
    // multi-GPU join next to its downsamples leaves a few more: the exchange's kernels need room too).
    static const int spare_knob = []() { const char *e = getenv("CWIPC_SPARE_CUS"); return e ? atoi(e) : -1; }();
    const int spare_cus = spare_knob >= 0 ? spare_knob : ws.cus / 32;
    cus = ws.cus - spare_cus > 8 ? ws.cus - spare_cus : ws.cus;
    // Clouds with few points per voxel fill the workgroup table (2048 voxels): the previous calls of this
    // thread tell (ws.shrink) how much smaller the workgroups have to be for it to hold; the extra
    // workgroups run one after the other on the same CUs.
    if (ws.hint_cell != cellsize || ws.hint_split != leaf_split || n > 2 * ws.hint_n || 2 * n < ws.hint_n) {   // another kind of cloud or call: start over
        ws.shrink = 0;
        ws.calm = 0;
        ws.incoherent = false;
        ws.no_fast = false;
        ws.streak = 0;
    }
    ws.hint_cell = cellsize;
    ws.hint_split = leaf_split;
    ws.hint_n = n;
    steps_total = (n + WAVE_STEP - 1) / WAVE_STEP;
    nwaves = general_plan_waves(n, cus, ws.shrink);
    nblocks = (uint32_t)(nwaves / K1_WAVES);

    memset(&P, 0, sizeof(P));
    P.n = n;
    P.per_wave = general_plan_per_wave(n, nwaves);
    P.nranges = (uint32_t)nwaves;
    P.leaf = cellsize;
    P.inv_leaf = 1.0f / cellsize;
    P.vox_unit = 1.0 / (double)P.inv_leaf;
    P.q_unit = P.vox_unit / 8388608.0;
    P.leaf_d = (double)cellsize;
    const float octree_cellsize = (8 * 8) * cellsize;   // reference src/cwipc_filters.cpp:113-114
    P.res = (double)octree_cellsize;
    P.leaf_split = leaf_split ? 1 : 0;
#ifdef CWIPC_DEBUG_KNOBS
    static const uint32_t ablate_knob = []() { const char *e = getenv("CWIPC_VOXEL_ABLATE"); return e ? (uint32_t)atoi(e) : 0u; }();   // read once
    if (ablate_knob) cwipc_log(CWIPC_LOG_LEVEL_WARNING, "cwipc_downsample", "CWIPC_VOXEL_ABLATE is set: results are WRONG (timing experiments only)");
    P.ablate = ablate_knob;
#endif
}

// Anchor and face thresholds (host, f64).  false: the call ends here, with `early` (nullptr: an error).
bool VoxCall::anchor_and_faces(std::shared_ptr<DeviceSoA> &early) {
    memset(faces_host, 0, sizeof(faces_host));
    if (leaf_split) {
        if (!fetch_first_point(src, c)) return false;
        float anchor[3] = {src.first[0], src.first[1], src.first[2]};
        if (!(std::isfinite(anchor[0]) && std::isfinite(anchor[1]) && std::isfinite(anchor[2]))) {
            // the octree skips non-finite points (addPointsFromInputCloud): its first point is the first finite one
            float *h = (float *)c.host_words;
            hipLaunchKernelGGL(first_finite_kernel, dim3(1), dim3(1024), 0, c.stream, src.x(), src.y(), src.z(), n, h);
            bool ok = hipGetLastError() == hipSuccess;
            ok = c.sync() && ok;
            if (!ok) { hip_failed(hipGetLastError(), "search for the first finite point", __FILE__, __LINE__); return false; }
            if (h[3] == 0.0f) { early = soa_alloc(0); return false; }   // no finite point at all: no leaves, an empty cloud
            anchor[0] = h[0]; anchor[1] = h[1]; anchor[2] = h[2];
        }
        const double pp[3] = {(double)anchor[0], (double)anchor[1], (double)anchor[2]};
        first_box(pp, P.res, P.mn0, P.mx0, P.depth0);
        for (int a = 0; a < 3; a++) {
            P.ib[a] = (int)floor(P.mn0[a] / P.leaf_d);
            // the first point sits in leaf 1 of its box: cover faces 1 - FACE_BACK .. 1 - FACE_BACK + FACES - 1
            P.face_base[a] = 1 - FACE_BACK;
        }
        // the thresholds depend on the anchor's box and the resolution only: a stream of frames of one scene
        // (and every repeat of a call) finds them in the workspace, host copy and device copy
        const bool cached = ws.faces_valid && ws.faces_res == P.res && ws.faces_mn0[0] == P.mn0[0] && ws.faces_mn0[1] == P.mn0[1] && ws.faces_mn0[2] == P.mn0[2];
        if (cached) {
            memcpy(faces_host, ws.faces_host, sizeof(faces_host));
        } else {
            fill_face_table(P.mn0, P.res, P.face_base, P.inv_leaf, faces_host);
        }
        faces_key_mn0[0] = P.mn0[0]; faces_key_mn0[1] = P.mn0[1]; faces_key_mn0[2] = P.mn0[2];
    } else {
        for (int a = 0; a < 3; a++) P.ib[a] = 2;   // bricks of 64 voxels aligned to the voxel lattice
    }
    return true;
}

bool VoxCall::partition_buffers() {
    // Points in no spatial order (learned from the calls before: the workgroup tables overflowed whatever the workgroup size):
    // move them into coarse spatial buckets first and accumulate the moved copy (voxel_partition.inc).
    static const bool partition_off = []() { const char *e = getenv("CWIPC_VOXEL_PARTITION"); return e && atoi(e) == 0; }();   // test knob
    partition = ws.incoherent && !partition_off && n >= 65536;
    const size_t part_stride = (n + 1023) & ~(size_t)1023;
    part_nseg = (nblocks + PART_SEG_ROWS - 1) / PART_SEG_ROWS;
    if (partition) {
        if (ws.part_stride < part_stride || ws.part_rows < nblocks) {
            ws.drop_partition_buffers();
            if (hipMalloc((void **)&ws.part, 16 * part_stride) != hipSuccess ||
                hipMalloc((void **)&ws.part_hist, ((size_t)nblocks + part_nseg + 1) * PART_BUCKETS * sizeof(uint32_t)) != hipSuccess) {
                (void)hipGetLastError();
                ws.drop_partition_buffers();
                hip_failed(hipErrorOutOfMemory, "voxel partition buffers", __FILE__, __LINE__);
                return false;
            }
            ws.part_stride = part_stride;
            ws.part_rows = nblocks;
            g_workspace_bytes += 16 * part_stride;
        }
    } else if (ws.part) {
        ws.drop_partition_buffers();   // (nothing of this workspace's stream is in flight: its last pass has reported above or long ago)
    }
    return true;
}

// How many leaf grids the first attempt gets; the grids go back first if the passes before used a fraction of them.
bool VoxCall::first_leaf_cap() {
    if (ws.shrink_to && ws.shrink_to < ws.leaf_cap) {
        // (this thread's last pass on the workspace may have its finalize kernel in flight still)
        if (!c.sync()) return false;
        ws.free_grids();
    }
    // 4 grids = 80 MB to begin with (a camera tile at 1 cm has 2 to 4 leaves, a person-sized cloud 12 to 16); x4 when a cloud has more
    leaf_cap = ws.leaf_cap ? ws.leaf_cap : (ws.shrink_to ? ws.shrink_to : 4);
    if (ws.shrink_to) ws.roomy = 0;
    ws.shrink_to = 0;
    return true;
}

// Workspace of the size this attempt needs, this pass's head block and sequence number, the face table on the device.
bool VoxCall::setup_pass() {
    if (!ensure_workspace(ws, n, leaf_cap, (uint32_t)nwaves, c.stream)) return false;
    P.leaf_mask = 4 * ws.leaf_cap - 1;
    P.list_cap = (uint32_t)(ws.list_cap > 0xffffffffu ? 0xffffffffu : ws.list_cap);
    seq = ++ws.seq ? ws.seq : ++ws.seq;
    for (int i = 0; i < C_SEQ; i++) ws.host_words[2 * i + 1] = 0;   // the tags of the words the replay kernel will publish
    // control words, leaf table, slice counts: this pass's block (zeroed by the previous pass's replay kernel)
    const int blk = ws.parity;
    char *head = ws.bind_head(blk);
    next_head = (char *)ws.head + (size_t)(1 - blk) * ws.head_bytes;
    W = ws.work();
    ok = true;
    if (!ws.head_clean[blk]) ok = hipMemsetAsync(head, 0, ws.head_bytes, c.stream) == hipSuccess;
    ws.head_clean[blk] = false;
    if (ok && mode == 1 && !(ws.faces_valid && memcmp(ws.faces_host, faces_host, sizeof(faces_host)) == 0)) {
        uint32_t *stage = (uint32_t *)c.staging(sizeof(faces_host));
        ok = stage != nullptr;
        if (ok) {
            memcpy(stage, faces_host, sizeof(faces_host));
            ok = hipMemcpyAsync(ws.faces, stage, sizeof(faces_host), hipMemcpyHostToDevice, c.stream) == hipSuccess;
            memcpy(ws.faces_host, faces_host, sizeof(faces_host));
            ws.faces_valid = ok;
            ws.faces_res = P.res;
            ws.faces_mn0[0] = faces_key_mn0[0]; ws.faces_mn0[1] = faces_key_mn0[1]; ws.faces_mn0[2] = faces_key_mn0[2];
        }
    }
    if (!ok) { hip_failed(hipGetLastError(), "voxel workspace setup", __FILE__, __LINE__); return false; }
    return true;
}

K1Params k1_params(const VoxParams &P, bool local_leaves) {
    K1Params K;
    memset(&K, 0, sizeof(K));
    K.n = (uint32_t)P.n; K.per_wave = (uint32_t)P.per_wave;
    K.inv_leaf = P.inv_leaf;
    K.ib0 = P.ib[0]; K.ib1 = P.ib[1]; K.ib2 = P.ib[2];
    K.fb0 = P.face_base[0]; K.fb1 = P.face_base[1]; K.fb2 = P.face_base[2];
    K.leaf_mask = P.leaf_mask; K.list_cap = P.list_cap; K.ablate = P.ablate;
    K.local_leaves = local_leaves ? 1u : 0u;
    K.want_list = P.leaf_split ? 0u : 1u;
    K.mn0[0] = P.mn0[0]; K.mn0[1] = P.mn0[1]; K.mn0[2] = P.mn0[2];
    K.res = P.res;
    return K;
}

FastParams fast_params(const K1Params &K, const FastPlan &plan) {
    FastParams F;
    memset(&F, 0, sizeof(F));
    F.n = K.n; F.per_wg = plan.per_wg; F.inv_leaf = K.inv_leaf;
    F.range_base_q = plan.base_q; F.range_inc_q = plan.inc_q;
    F.ib0 = K.ib0; F.ib1 = K.ib1; F.ib2 = K.ib2;
    F.fb0 = K.fb0; F.fb1 = K.fb1; F.fb2 = K.fb2;
    F.leaf_mask = K.leaf_mask; F.list_cap = K.list_cap; F.want_list = K.want_list;
    return F;
}

// The accumulate kernel, fast or general, with the partition pass in front of it for a cloud in no spatial order.
void VoxCall::launch_accumulate() {
    const K1Params K = k1_params(P, local_leaves);
    // The fast variant takes coherent clouds that fit its workgroup table and key; it says so (ERR_FAST_PATH) when a
    // cloud does not, and the pass is run again with the general variant (which is remembered for the clouds to come).
    static const bool fast_off = []() { const char *e = getenv("CWIPC_VOXEL_GENERAL"); return e && atoi(e) != 0; }();   // test knob: general variant only
    const bool fast = mode != 2 && !ws.no_fast && ws.shrink == 0 && !fast_off && !partition;
    // the planes the accumulate kernel reads, and where it leaves its boxes
    const float *kx = src.x(), *ky = src.y(), *kz = src.z();
    const uint32_t *kw = src.rgbt();
    VoxWork Wk = W;
    if (partition) {
        float *px = ws.part, *py = px + ws.part_stride, *pz = py + ws.part_stride;
        uint32_t *pw = (uint32_t *)(pz + ws.part_stride);
        const uint32_t padded = (uint32_t)((n + WAVE_STEP - 1) / WAVE_STEP * WAVE_STEP);
        // the table: rows [part_rows][buckets], then the segments' sums [nseg][buckets], then the buckets' starts (every word is
        // written by the kernels that follow: nothing to clear)
        uint32_t *rows = ws.part_hist, *seg = rows + ws.part_rows * PART_BUCKETS, *start = seg + part_nseg * PART_BUCKETS;
        const uint32_t per_wg = (uint32_t)(P.per_wave * K1_WAVES);
        CW_LAUNCH("partition_count", partition_count_kernel, dim3(nblocks), dim3(K1_THREADS), 0, c.stream, (uint32_t)n, per_wg, P.inv_leaf,
                  src.x(), src.y(), src.z(), ws.bboxes, rows, ws.ctrl);
        CW_LAUNCH("partition_scan", partition_segsum_kernel, dim3((unsigned)part_nseg, PART_BUCKETS / 256), dim3(256), 0, c.stream, rows, nblocks, seg);
        CW_LAUNCH("partition_scan", partition_starts_kernel, dim3(1), dim3(K1_THREADS), 0, c.stream, seg, (uint32_t)part_nseg, start);
        CW_LAUNCH("partition_scatter", partition_scatter_kernel, dim3(nblocks), dim3(K1_THREADS), sizeof(PartLds), c.stream,
                  (uint32_t)n, per_wg, padded, P.inv_leaf, src.x(), src.y(), src.z(), src.rgbt(), px, py, pz, pw, rows, seg, start);
        kx = px; ky = py; kz = pz; kw = pw;
        Wk.bboxes = ws.bboxes + (size_t)ws.bbox_cap * 6;   // the boxes of the moved points: nobody reads them
    }
    used_fast = fast;
    fplan = FastPlan{0u, 0u, 0u, 0u};
    if (fast) {
        // (the ranges: voxel_anchor.hpp, fast_plan)
        static const int stagger_knob = []() { const char *e = getenv("CWIPC_K1_STAGGER"); return e ? atoi(e) : 25; }();
        fplan = fast_plan(n, cus, stagger_knob);
        FastParams F = fast_params(K, fplan);
#ifdef CWIPC_DEBUG_KNOBS
        static const uint32_t fast_dbg = []() { const char *e = getenv("CWIPC_FAST_DBG"); return e ? (uint32_t)atoi(e) : 0u; }();
        if (fast_dbg) cwipc_log(CWIPC_LOG_LEVEL_WARNING, "cwipc_downsample", "CWIPC_FAST_DBG is set: results are WRONG (timing experiments only)");
        F.dbg = fast_dbg;
#endif
        if (mode == 0) {
            CW_LAUNCH("voxel_accumulate", voxel_accumulate_fast_kernel<0>, dim3(fplan.blocks), dim3(K1_THREADS), sizeof(FastTable), c.stream, F, src.x(),
                      src.y(), src.z(), src.rgbt(), W);
        } else {
            CW_LAUNCH("voxel_accumulate", voxel_accumulate_fast_kernel<1>, dim3(fplan.blocks), dim3(K1_THREADS), sizeof(FastTable), c.stream, F, src.x(),
                      src.y(), src.z(), src.rgbt(), W);
        }
    } else if (mode == 0) {
        CW_LAUNCH("voxel_accumulate_general", voxel_accumulate_kernel<0>, dim3(nblocks), dim3(K1_THREADS), sizeof(LdsTable), c.stream, K, kx, ky, kz, kw, Wk);
    } else if (mode == 1) {
        CW_LAUNCH("voxel_accumulate_general", voxel_accumulate_kernel<1>, dim3(nblocks), dim3(K1_THREADS), sizeof(LdsTable), c.stream, K, kx, ky, kz, kw, Wk);
    } else {
        CW_LAUNCH("voxel_accumulate_exact", voxel_accumulate_kernel<2>, dim3(nblocks), dim3(K1_THREADS), sizeof(LdsTable), c.stream, K, kx, ky, kz, kw, Wk);
    }
}

void VoxCall::launch_replay() {
    // (the fast variant and the partition pass leave one box per workgroup range, the general variant one per wave range)
    VoxParams Pr = P;
    if (used_fast) {
        Pr.per_wave = fplan.per_wg;
        Pr.nranges = fplan.blocks;
        Pr.range_base_q = fplan.base_q; Pr.range_inc_q = fplan.inc_q;
    } else if (partition) {   // the counting kernel's boxes: one per workgroup range of the cloud as it came
        Pr.per_wave = P.per_wave * K1_WAVES;
        Pr.nranges = nblocks;
    }
    CW_LAUNCH("octree_replay", octree_replay_kernel, dim3(1), dim3(1024), 0, c.stream, Pr, src.x(), src.y(), src.z(), ws.bboxes, ws.ctrl,
              ws.leaf_keys, ws.leaf_cap, (uint32_t *)next_head, (uint32_t)(ws.head_bytes / 4), ws.host_words, seq);
    launch_err = hipGetLastError();
    ok = launch_err == hipSuccess;
    const int blk = ws.parity;
    ws.head_clean[1 - blk] = ok;
    ws.parity = 1 - blk;
}

// The plain grid's five finalize passes (mark, block counts, block scan, emit, unmark) over `count` records and `words` words of the
// index bitmap.  spec.on == 0: the counts are the pass's own, known to the host; else they are the room provided, the kernels
// take the real ones from the control block, and the launches are not profiled (a speculative launch never is).
void VoxCall::launch_grid_finalize(const GridSpec &spec, uint32_t count, uint32_t words, DeviceSoA &dst) {
    const bool prof = !spec.on;
#define GRID_LAUNCH(name, ...) do { if (prof) CW_LAUNCH(name, __VA_ARGS__); else hipLaunchKernelGGL(__VA_ARGS__); } while (0)
    const uint32_t m_host = spec.on ? 0u : count, nwords_host = spec.on ? 0u : words;
    const unsigned mgrid = (count + 255) / 256, nblk = (unsigned)((words + GB_WORDS_PER_BLOCK - 1) / GB_WORDS_PER_BLOCK);
    GRID_LAUNCH("grid_mark", grid_mark_kernel, dim3(mgrid), dim3(256), 0, c.stream, P, W, m_host, spec, ws.gbits, ws.order);
    GRID_LAUNCH("grid_block", grid_block_kernel, dim3(nblk), dim3(256), 0, c.stream, W, spec, ws.gbits, nwords_host, ws.gprefix, ws.gblock);
    GRID_LAUNCH("grid_blockscan", grid_blockscan_kernel, dim3(1), dim3(1024), 0, c.stream, W, spec, ws.gblock, nwords_host);
    GRID_LAUNCH("grid_emit", grid_emit_kernel, dim3(mgrid), dim3(256), 0, c.stream, P, W, m_host, spec, ws.order, ws.gbits, ws.gprefix, ws.gblock,
                dst.x(), dst.y(), dst.z(), dst.rgbt());
    GRID_LAUNCH("grid_unmark", grid_unmark_kernel, dim3(mgrid), dim3(256), 0, c.stream, W, m_host, spec, ws.order, ws.gbits);
#undef GRID_LAUNCH
}

// The finalize pass before the host knows the outcome of the pass, into a result sized from the thread's last call.
void VoxCall::launch_speculative() {
    // Octree variant: the finalize pass goes out right behind the replay kernel, before the host knows the
    // count, into a result sized from the previous call of this thread (+25 %); it checks count and error
    // word on the device and leaves everything untouched if they do not fit.
    spec_dst.reset();
    spec_cap = 0;
    if (ok && leaf_split && ws.last_m > 0 && !profiling_enabled()) {
        spec_cap = ws.last_m + ws.last_m / 4 + 1024;
        spec_dst = soa_alloc(spec_cap);
        if (spec_dst) {
            hipLaunchKernelGGL(rank_emit_kernel, dim3(ws.leaf_cap * RANK_SEGS), dim3(RANK_THREADS), 0, c.stream, P, W, ws.leaf_cap, spec_cap, 1, ws.order,
                               spec_dst->x(), spec_dst->y(), spec_dst->z(), spec_dst->rgbt());
            // its `ready` event now, while the kernels run, not after the wait below: what the host does
            // between the end of that wait and the next call's first launch is time the GPU stands still
            spec_dst->mark_pending(c.stream);
        }
    }
    // Plain grid: the same, five small kernels instead of one (mark, block counts, block scan, emit, unmark), with
    // room for last call's count (+25 %) and the index bitmap as it stands; each of them checks on the device
    // that the pass succeeded and fits, and does nothing otherwise.
    gspec = GridSpec{0, 0u, 0u, 0ull};
    bitmap_max = GRID_BITMAP_MAX_CELLS;
    if (const char *e = getenv("CWIPC_GRID_BITMAP_MAX")) bitmap_max = strtoull(e, nullptr, 10);   // test knob: force the sort path
    if (ok && !leaf_split && ws.last_m_grid > 0 && ws.gwords_cap > 0 && !profiling_enabled()) {
        spec_cap = ws.last_m_grid + ws.last_m_grid / 4 + 1024;
        if (spec_cap > P.list_cap) spec_cap = P.list_cap;
        spec_dst = soa_alloc(spec_cap);
        if (spec_dst) {
            gspec = GridSpec{1, spec_cap, (uint32_t)std::min<size_t>(ws.gwords_cap, 0xffffffffu), bitmap_max};
            launch_grid_finalize(gspec, spec_cap, gspec.words_cap, *spec_dst);
            spec_dst->mark_pending(c.stream);
        }
    }
}

// A stream of frames (the two passes before went through at the first attempt): the call returns here, with its
// kernels in flight (r3: the plain grid's seven too).  The host does not wait for the count any more, so the next call's accumulate kernel
// is queued while this pass's replay and finalize kernels still run (on the thread's other stream), and the
// 15 us that lay between two accumulate kernels (replay kernel + the host's return, next entry and launch) are gone.
// true: handed out, the call returns.
bool VoxCall::hand_out(int attempt, std::shared_ptr<DeferredResult> *deferred) {
    static const bool defer_on = []() { const char *e = getenv("CWIPC_DEFER"); return !e || atoi(e) != 0; }();
    if (!(deferred && defer_on && attempt == 0 && ok && spec_dst && (leaf_split || gspec.on) && ws.streak >= 2)) return false;
    auto p = std::make_shared<PendingVoxel>();
    p->src = src_ptr;
    p->spec_dst = spec_dst;
    p->words = reinterpret_cast<volatile unsigned long long *>(ws.host_words);
    p->stream = c.stream;
    p->seq = seq;
    p->spec_cap = spec_cap;
    p->cellsize = cellsize;
    p->leaf_split = leaf_split;
    p->gspec = gspec;
    p->partitioned = partition;
    p->steps_total = (uint32_t)steps_total;
    src.note_reader(c.stream);   // the input's planes are not recycled before the accumulate kernel is done with them
    ws.pending = p;
    *deferred = p;
    return true;
}

// wait for the replay kernel's sequence number in pinned memory (a few hundred microseconds of
// polling at most, then the ordinary stream wait, which also reports launch failures)
PassReport VoxCall::await_report() {
    volatile unsigned long long *words = reinterpret_cast<volatile unsigned long long *>(ws.host_words);
    const PassReport hw = read_report(words, seq, ok && !profiling_enabled(), [&]() { ok = c.sync() && ok; return ok; });
    if (ok && !hw.seen) { ok = false; cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_downsample", "voxel grid failed: the replay kernel did not report"); }
    return hw;
}

#ifdef CWIPC_DEBUG_KNOBS
// CWIPC_FAST_STAMPS: the fast accumulate kernel's phase time stamps, logged
void log_fast_stamps(uint32_t fast_blocks) {
    unsigned long long st[2][16];
    (void)hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(st, HIP_SYMBOL(g_fast_stamps), sizeof(st)) == hipSuccess) {
        for (int w = 0; w < 2; w++) {
            std::string line = "debug: workgroup " + std::string(w ? "mid" : "0") + " phases (us since its start): ";
            const char *names[9] = {"start", "table ready", "steps done", "boxes out", "entries compacted", "keys decoded", "leaf ids", "records updated", "end"};
            for (int i = 1; i < 9; i++) line += std::string(names[i]) + " " + std::to_string((double)(st[w][i] - st[w][0]) * 0.01).substr(0, 5) + "; ";
            cwipc_log(CWIPC_LOG_LEVEL_WARNING, "cwipc_downsample", line);
        }
        static unsigned long long wt[1024][4];
        if (hipMemcpyFromSymbol(wt, HIP_SYMBOL(g_wg_times), sizeof(wt)) == hipSuccess && fast_blocks > 0 && fast_blocks <= 1024) {
            unsigned long long t0 = ~0ull, s_max = 0, e_min = ~0ull, e_max = 0, d_min = ~0ull, d_max = 0, a_max = 0;
            for (uint32_t b = 0; b < fast_blocks; b++) {
                t0 = std::min(t0, wt[b][0]); s_max = std::max(s_max, wt[b][0]);
                e_min = std::min(e_min, wt[b][3]); e_max = std::max(e_max, wt[b][3]);
                d_min = std::min(d_min, wt[b][3] - wt[b][0]); d_max = std::max(d_max, wt[b][3] - wt[b][0]);
                a_max = std::max(a_max, wt[b][2]);
            }
            char buf[256];
            snprintf(buf, sizeof(buf), "debug: %u workgroups: last start %.2f us after the first; records updated between %.2f and %.2f us; all waves done by %.2f; a workgroup lives %.2f to %.2f us",
                     fast_blocks, (double)(s_max - t0) * 0.01, (double)(e_min - t0) * 0.01, (double)(e_max - t0) * 0.01, (double)(a_max - t0) * 0.01, (double)d_min * 0.01, (double)d_max * 0.01);
            cwipc_log(CWIPC_LOG_LEVEL_WARNING, "cwipc_downsample", buf);
            if (const char *path = getenv("CWIPC_FAST_STAMPS_FILE")) {   // every workgroup's row, for a look at the spread
                if (FILE *f = fopen(path, "w")) {
                    fprintf(f, "# workgroup start stream_done(thread 0's wave) all_waves_done end   (us since the first start)\n");
                    for (uint32_t b = 0; b < fast_blocks; b++)
                        fprintf(f, "%u %.2f %.2f %.2f %.2f\n", b, (double)(wt[b][0] - t0) * 0.01, (double)(wt[b][1] - t0) * 0.01, (double)(wt[b][2] - t0) * 0.01, (double)(wt[b][3] - t0) * 0.01);
                    fclose(f);
                }
            }
        }
        unsigned long long wd[K1_WAVES];
        if (hipMemcpyFromSymbol(wd, HIP_SYMBOL(g_fast_wave_done), sizeof(wd)) == hipSuccess) {
            std::string line = "debug: workgroup 0, waves done with their steps at (us):";
            for (int w = 0; w < K1_WAVES; w++) line += " " + std::to_string((double)(wd[w] - st[0][0]) * 0.01).substr(0, 5);
            cwipc_log(CWIPC_LOG_LEVEL_WARNING, "cwipc_downsample", line);
        }
    }
}
#endif

// The workgroup size of the next call, from how the workgroup tables fared (a pass without the partition pass in front).
void VoxCall::adapt_workgroups(const PassReport &hw) {
    const uint32_t fallbacks = hw[C_FALLBACK], maxload = hw[C_MAXLOAD];
    if (!used_fast && !err && n >= 65536 && 2 * ((size_t)hw[C_FLUSHED] + fallbacks) > n && n > 4 * (size_t)hw[C_COUNT]) {
        // Voxels hold several points each, and yet most points went to the global records on their own (a cloud in scan
        // order: one update per ~90 points at the 10 M configuration): the workgroups' ranges are all over the place.
        // The partition pass takes such clouds from the next call on.
        ws.incoherent = true;
        ws.shrink = 0;
        ws.calm = 0;
    } else if (ws.incoherent) {
        // nothing to adapt: this kind of cloud defeats the table whatever its size
    } else if (ws.shrink >= 2 && (size_t)fallbacks * 2 > n) {
        ws.incoherent = true;   // smaller workgroups did not help: points in no order at all
        ws.shrink = 0;
        ws.calm = 0;
    } else if ((size_t)fallbacks * 64 > n && ws.shrink < 6) {
        ws.shrink++;
        ws.calm = 0;
    } else if (ws.shrink > 0 && fallbacks == 0 && maxload * 3 < (uint32_t)LTAB) {
        if (++ws.calm >= 4) { ws.shrink--; ws.calm = 0; }
    } else {
        ws.calm = 0;
    }
}

// The result of a pass whose report is in: the speculative one if its kernels ran, else the finalize kernels now; after an
// error only the clean-up, for the records must be left zeroed either way.
std::shared_ptr<DeviceSoA> VoxCall::finalize(const PassReport &hw, uint32_t m) {
    std::shared_ptr<DeviceSoA> dst;
    unsigned long long *keys_in = nullptr, *keys_out = nullptr;
    uint32_t *vals_in = nullptr, *vals_out = nullptr;
    void *sort_tmp = nullptr;
    const unsigned mgrid = (m + 255) / 256;

    bool ranked = false;
    bool grid_ranked = false;
    if (!err && m && !leaf_split && spec_dst && gspec.on && grid_fits(hw, gspec)) {
        dst = spec_dst;
        dst->npoints = m;
        grid_ranked = true;
    }
    if (!err && m && leaf_split && spec_dst && m <= spec_cap) {
        // the speculative finalize pass is doing the work: the result uses the first m slots of its planes
        dst = spec_dst;
        dst->npoints = m;
        ranked = true;
    }
    spec_dst.reset();
    if (!ranked && !err && m && leaf_split) {
        // octree path: rank the occupied cells through the bitmaps, emit, clean -- no sort.  The
        // replay kernel has already checked everything this pass could trip over, so the call
        // returns with it in flight: the result carries a `ready` event, later work of this thread
        // (including the next call's use of the workspace) is ordered behind it on the stream.
        dst = soa_alloc(m);
        if (!dst) {
            err |= 0x80000000u;
        } else {
            CW_LAUNCH("rank_emit", rank_emit_kernel, dim3(ws.leaf_cap * RANK_SEGS), dim3(RANK_THREADS), 0, c.stream, P, W, ws.leaf_cap, m, 0, ws.order,
                      dst->x(), dst->y(), dst->z(), dst->rgbt());
            dst->mark_pending(c.stream);
            ranked = true;
        }
    }
    if (!err && m && !leaf_split && !grid_ranked) {
        // plain grid, the usual case: output order from a bitmap over the VoxelGrid index space, no sort;
        // like the octree variant the call returns with these passes in flight
        const unsigned long long cells = (unsigned long long)hw[C_DIVB] * hw[C_DIVB + 1] * hw[C_DIVB + 2];
        if (cells <= bitmap_max) {
            const uint32_t nwords = (uint32_t)((cells + 31) / 32);
            bool ready = true;
            if (ws.gwords_cap < nwords) {
                ws.free_index_bitmap();
                const size_t cap = std::max<size_t>((size_t)nwords * 2, (size_t)1 << 16);
                ready = hipMalloc((void **)&ws.gbits, cap * 4) == hipSuccess && hipMalloc((void **)&ws.gprefix, cap * 4) == hipSuccess &&
                        hipMalloc((void **)&ws.gblock, (cap / GB_WORDS_PER_BLOCK + 2) * 4) == hipSuccess &&
                        hipMemsetAsync(ws.gbits, 0, cap * 4, c.stream) == hipSuccess;
                if (ready) ws.gwords_cap = cap; else (void)hipGetLastError();
            }
            dst = ready ? soa_alloc(m) : nullptr;
            if (dst) {
                launch_grid_finalize(GridSpec{0, 0u, 0u, 0ull}, m, nwords, *dst);
                dst->mark_pending(c.stream);
                grid_ranked = true;
            }
        }
    }
    if (!err && m && !leaf_split && !grid_ranked) {
        // index spaces beyond 2^28 cells: sort the touched records by index
        dst = soa_alloc(m);
        keys_in = (unsigned long long *)pool_alloc((size_t)m * 8 * 2);
        vals_in = (uint32_t *)pool_alloc((size_t)m * 4 * 2);
        if (!dst || !keys_in || !vals_in) {
            err |= 0x80000000u;
        } else {
            keys_out = keys_in + m;
            vals_out = vals_in + m;
            CW_LAUNCH("make_sort_keys", make_sort_keys_kernel, dim3(mgrid), dim3(256), 0, c.stream, P, W, m, keys_in, vals_in);
            // only the bits that can be set take part in the sort
            const unsigned end_bit = 32;   // idx < 2^31
            size_t tmp_bytes = 0;
            hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)m, 0u, end_bit, c.stream);
            if (e == hipSuccess) {
                sort_tmp = pool_alloc(tmp_bytes ? tmp_bytes : 256);
                if (!sort_tmp) e = hipErrorOutOfMemory;
            }
            if (e == hipSuccess) {
                if (profiling_enabled()) profile_begin("radix_sort_pairs", c.stream);
                e = rocprim::radix_sort_pairs(sort_tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)m, 0u, end_bit, c.stream);
                if (profiling_enabled()) profile_end(c.stream);
            }
            if (e != hipSuccess) {
                hip_failed(e, "rocprim::radix_sort_pairs", __FILE__, __LINE__);
                err |= 0x80000000u;
            }
        }
    }
    if (leaf_split && !ranked) {
        // octree variant, error: the records must be left zeroed
        CW_LAUNCH("clean_by_bitmap", clean_by_bitmap_kernel, dim3(ws.leaf_cap * RANK_SEGS), dim3(RANK_THREADS), 0, c.stream, W);
        ok = c.sync() && ok;
    }
    if (!leaf_split && m && !grid_ranked) {
        // emit (or, on error, only clean): the records must be left zeroed either way
        const int emit = (!err && dst) ? 1 : 0;
        CW_LAUNCH("emit_and_clean", emit_and_clean_kernel, dim3(mgrid), dim3(256), 0, c.stream, P, W, m, vals_out, emit ? dst->x() : nullptr,
                  emit ? dst->y() : nullptr, emit ? dst->z() : nullptr, emit ? dst->rgbt() : nullptr, emit);
        if (emit) ok = hipMemcpyAsync(c.host_words, ws.ctrl, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
        ok = c.sync() && ok;
        if (emit && ok) err |= c.host_words[C_ERR];
    }
    pool_free(keys_in);
    pool_free(vals_in);
    pool_free(sort_tmp);
    return dst;
}

// true: run the pass again with what was too small changed; false: `dst` is the call's result (nullptr after an error).
bool VoxCall::retry_or_report(int attempt, const PassReport &hw, uint32_t m, std::shared_ptr<DeviceSoA> &dst) {
    const uint32_t retryable = ERR_LEAVES | ERR_FACE_TABLE | ERR_LOCAL_LEAVES | ERR_LIST_FULL | ERR_FAST_PATH | (used_fast ? ERR_CELL_RANGE : 0u);
    if (used_fast && (err & (ERR_FAST_PATH | ERR_CELL_RANGE)) && !(err & ~retryable)) {
        // not a cloud for the fast variant (its table, its key or its slabs): the touched records were cleaned above
        ws.no_fast = true;
        return true;
    }
    if ((err & (ERR_LEAVES | ERR_FACE_TABLE | ERR_LOCAL_LEAVES)) && !(err & ~retryable)) {
        if (err & ERR_LOCAL_LEAVES) local_leaves = false;   // a workgroup spans more than 64 leaves: global ids in the hot loop
        // the touched records were cleaned above; change what was too small and run again
        if (err & ERR_FACE_TABLE) mode = 2;   // points beyond the threshold table: per-point f64 variant
        if (err & ERR_LEAVES) {
            if ((size_t)leaf_cap * 4 * GRID_BYTES > ((size_t)200 << 30)) {
                cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_downsample", "voxel grid failed: the cloud spans more octree leaves than fit in device memory");
                dst = nullptr;
                return false;
            }
            leaf_cap *= 4;
        }
        return true;
    }
    if (err) {
        std::string why;
        if (err & ERR_GRID_OVERFLOW) why += " VoxelGrid: leaf size is too small for the input dataset, integer indices would overflow;";
        if (err & ERR_RANGE) why += " voxel or leaf index out of range;";
        if (err & (ERR_DEPTH | ERR_LEAF_RANGE)) why += " octree deeper than 14 levels;";
        if (err & ERR_CELL_RANGE) why += " voxel outside its leaf grid;";
        if (err & ERR_LIST_FULL) why += " occupied list full;";
        if (err & 0x80000000u) why += " device allocation or sort failure;";
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_downsample", "voxel grid failed:" + why);
        dst = nullptr;
        return false;
    }
    if (!m) {
        dst = empty_result(leaf_split);
        return false;
    }
    ws.streak = attempt == 0 ? ws.streak + 1 : 0;
    ws.note_leaves(hw[C_LEAVES]);
    return false;
}

}  // namespace

// "Is the workspace whose turn it is still at work?" is asked of its stream -- and has to be asked BEFORE the call orders that stream
// behind the producer of its input: a cloud that came out of another filter with its last kernel still running (r4: colorize, as
// a join's result since round 2) puts a wait into the thread's first stream, which then reads as busy although the workspace has
// been idle since the frame before, and every thread of a per-tile chain took a second and a third workspace (0.3 GB each) for
// calls that could not overlap anyway.  cwipc_downsample samples the streams on entry; the call that follows uses the sample.
void voxel_sample_streams() {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return;
    uint32_t bits = 0;
    for (int i = 0; i < MAX_WS && t_ws.ws[i]; i++) {
        hipStream_t s = workspace_stream(c, i);
        if (s && hipStreamQuery(s) == hipErrorNotReady) bits |= 1u << i;
        (void)hipGetLastError();   // (hipErrorNotReady is an answer, not a failure)
    }
    t_busy_sample = bits;
    t_busy_sampled = true;
}

std::shared_ptr<DeviceSoA> voxel_downsample(const std::shared_ptr<DeviceSoA> &src_ptr, float cellsize, bool leaf_split, int *error_code,
                                            std::shared_ptr<DeferredResult> *deferred) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return nullptr;
    const int which = pick_workspace(c);
    Workspace &ws = t_ws.get(which);
    StreamOfWorkspace on_its_stream(c, which);
    VoxCall k(c, ws, src_ptr, cellsize, leaf_split);
    if (!k.collect_pending()) return nullptr;
    k.src.wait_on(c.stream);   // (the caller ordered the thread's first stream behind the input's producer; this may be the second)
    if (k.n >= ((size_t)1 << 31)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_downsample", "voxel grid failed: more than 2^31 points");
        return nullptr;
    }
    k.plan();
    std::shared_ptr<DeviceSoA> result;
    if (!k.anchor_and_faces(result)) return result;
    if (!k.partition_buffers() || !k.first_leaf_cap()) return nullptr;
    for (int attempt = 0; attempt < 10; attempt++) {
        if (!k.setup_pass()) return nullptr;
        k.launch_accumulate();
        k.launch_replay();
        k.launch_speculative();
        if (k.hand_out(attempt, deferred)) return nullptr;
        const PassReport hw = k.await_report();
        if (!k.ok) { hip_failed(k.launch_err != hipSuccess ? k.launch_err : hipGetLastError(), "voxel_accumulate", __FILE__, __LINE__); return nullptr; }
        k.err = hw[C_ERR];
#ifdef CWIPC_DEBUG_KNOBS
        if (k.used_fast && getenv("CWIPC_FAST_STAMPS")) log_fast_stamps(k.fplan.blocks);
#endif
        const uint32_t m = hw[C_COUNT] < k.P.list_cap ? hw[C_COUNT] : k.P.list_cap;
        learn_from_pass(ws, leaf_split, !k.err, m, k.partition, hw[C_SCATTER], k.steps_total);
        if (!k.partition) k.adapt_workgroups(hw);
        result = k.finalize(hw, m);
        if (error_code) *error_code = (int)k.err;
        if (!k.ok) { hip_failed(hipGetLastError(), "voxel emit", __FILE__, __LINE__); return nullptr; }
        if (!k.retry_or_report(attempt, hw, m, result)) return result;
    }
    cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_downsample", "voxel grid failed: could not size the workspace");
    return nullptr;
}

size_t voxel_workspace_bytes() { return g_workspace_bytes.load(); }

// The workspaces that threads which have ended left for the next threads (at most eight) go back to the device.  For a
// deployment that wants the memory back after a burst of threads, and for tests that measure a footprint.
size_t voxel_release_pooled_workspaces() {
    std::vector<Workspace *> gone;
    {
        std::lock_guard<std::mutex> lock(g_ws_pool_mutex);
        gone.swap(*g_ws_pool);
    }
    if (!gone.empty()) (void)hipDeviceSynchronize();
    for (Workspace *w : gone) {
        if (w->pending) (void)w->pending->outcome();   // (a result somebody still holds reads its report from this workspace's words)
        delete w;
    }
    return gone.size();
}

}  // namespace cwipc_amd

extern "C" _CWIPC_UTIL_EXPORT size_t cwipc_hip_workspace_bytes(void) { return cwipc_amd::voxel_workspace_bytes(); }
extern "C" _CWIPC_UTIL_EXPORT size_t cwipc_hip_workspace_trim(void) { return cwipc_amd::voxel_release_pooled_workspaces(); }
