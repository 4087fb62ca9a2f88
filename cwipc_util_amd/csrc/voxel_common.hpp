// voxel_common.hpp -- what the parts of the voxel-grid downsample share (kernels_voxel.hip names them): constants, error bits and
// control words, the parameter blocks, the leaf table and the records.  The host part (everything above the device functions) also
// compiles with the host C++ compiler alone: tests/abi/voxel_anchor_host.cpp reads the constants and range_first_step from here.
#pragma once
#include <cstddef>
#include <cstdint>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_HOST_DEVICE __host__ __device__
#else
#define CWIPC_HOST_DEVICE
#endif
namespace cwipc_amd {
namespace {

// ---------------------------------------------------------------------------
// constants and shared structures
// ---------------------------------------------------------------------------
constexpr int K1_THREADS = 1024;
constexpr int K1_WAVES = K1_THREADS / 64;
constexpr int WAVE_STEP = 256;                 // points per wave per step (4 per lane)
constexpr size_t MAX_POINTS_PER_WAVE = 3840;   // 15 steps; 16 waves -> at most 61440 points per workgroup
constexpr int LTAB = 2048;                     // LDS table entries per workgroup
constexpr int LTAB_PROBES = 32;
constexpr int GRID_DIM = 68;                   // cells per axis of a leaf grid (64 + slack for fp rounding)
constexpr int CELLS = GRID_DIM * GRID_DIM * GRID_DIM;   // 314432 < 2^19
constexpr int CELL_BITS = 19;
constexpr int BITWORDS = CELLS / 32;            // 9826 occupancy words per leaf grid (CELLS is a multiple of 32)
constexpr uint32_t KEY_EMPTY = 0xffffffffu;
constexpr int HIST = 256;                      // slots of the per-workgroup histogram of first touches per bitmap slice
constexpr int LOCAL_LEAVES = 64;               // leaves a workgroup can name locally (keys carry the local slot, the flush translates)
// the finalize pass works on slices of a leaf's occupancy bitmap
constexpr int RANK_THREADS = 256;
constexpr int RANK_SEGS = 16;                  // a few leaves hold all the work: many slices per leaf for enough workgroups
constexpr int SEG_WORDS = (BITWORDS + RANK_SEGS - 1) / RANK_SEGS;                 // 615
constexpr int WORDS_PER_THREAD = (SEG_WORDS + RANK_THREADS - 1) / RANK_THREADS;   // 3
constexpr int RECORD_WORDS = 8;                // 64-byte records: sx sy sz cr gb tlo thi tor
constexpr int FACES = 128;                     // leaf faces per axis with a precomputed threshold
constexpr int FACE_BACK = 63;                  // the table starts 63 faces below the first point's leaf
// threshold table in 32-bit words: [3][FACES] thresholds T (float), [3][FACES] Tv (float: lower bound of the voxel above
// the one T lies in), [3][FACES] tf (int: index of the voxel T lies in); the general kernel reads the first part only
constexpr int FT_T = 0, FT_TV = 3 * FACES, FT_TF = 6 * FACES, FACE_TABLE_WORDS = 9 * FACES;

enum : uint32_t {
    ERR_RANGE = 1,           // voxel index outside +-2^26, or leaf index outside +-2^20
    ERR_LEAVES = 2,          // more octree leaves than the workspace has grids for (host regrows and retries)
    ERR_DEPTH = 4,           // octree deeper than the sort key can express
    ERR_GRID_OVERFLOW = 8,   // pcl::VoxelGrid: "Leaf size is too small ... indices would overflow"
    ERR_LEAF_RANGE = 16,
    ERR_FACE_TABLE = 32,     // a point lies beyond the threshold table (host reruns the exact variant)
    ERR_CELL_RANGE = 64,
    ERR_LIST_FULL = 128,
    ERR_LOCAL_LEAVES = 512,  // a workgroup met more leaves than its local leaf table holds: host reruns with global leaf ids in the hot loop
    ERR_FAST_PATH = 1024,    // the fast variant cannot take this cloud (host reruns the general variant)
};

// control block, 32-bit words in device memory
enum {
    C_ERR = 0, C_COUNT = 1, C_DEPTH = 2, C_EVENTS = 3, C_SHIFT = 4 /* 3 x int64 */, C_MINB = 10, C_DIVB = 13,
    C_FALLBACK = 16,   // runs that found the workgroup table full and went to the global records one lane at a time
    C_MAXLOAD = 17,    // fullest workgroup table (entries)
    C_SCATTER = 18,    // partition pass: wave steps of the cloud as it came whose points spread over many buckets
    C_FLUSHED = 19,    // table entries flushed by all workgroups = global record updates of the pass (the general variant counts them)
    C_LEAVES = 20,     // octree leaves (or bricks of the plain grid) the pass has met = leaf grids in use
    C_SEQ = 31,        // number of published words (the host copy carries the pass's sequence number in the upper half of each 64-bit word)
    C_WORDS = 32
};

struct VoxParams {
    size_t n;
    size_t per_wave;        // points per wave range (multiple of WAVE_STEP)
    uint32_t range_base_q, range_inc_q;   // != 0: the ranges the replay kernel gets boxes of have growing lengths (range_first_step)
    uint32_t nranges;       // number of wave ranges = waves in the K1 grid
    float inv_leaf;         // 1 / leaf in fp32, as pcl::VoxelGrid::setLeafSize
    float leaf;
    double leaf_d;
    double vox_unit;        // 1 / inv_leaf: a voxel index times this is the voxel's lower corner
    double q_unit;          // 1 / (inv_leaf * 2^23): what one unit of the offset sums is worth
    double res;             // octree resolution (double)(float)(64 * leaf)
    // anchor (host): first octree box and the voxel index of its lower corner
    double mn0[3], mx0[3];
    int depth0;
    int ib[3];              // cell c of leaf l on axis a is voxel  c + ib[a] + 64*l - 2
    int face_base[3];       // faces[a][i] is the threshold of face face_base[a] + i
    int leaf_split;
    uint32_t leaf_mask;     // capacity of the leaf hash - 1 (the hash has four slots per leaf grid)
    uint32_t list_cap;
    uint32_t ablate;        // diagnostics only (CWIPC_VOXEL_ABLATE): skip parts of K1 to time the rest; results are wrong when non-zero
};

struct VoxWork {
    unsigned long long *leaf_keys;   // [leaf id] 0 = none yet, else packed lattice coordinates | 1<<63 (ids are handed out in order of arrival)
    unsigned long long *records;     // [leaf hash][CELLS][8]
    uint32_t *occupied;              // list of (leaf id << 19 | cell) of touched records
    uint32_t *ctrl;
    float *bboxes;                   // [nranges][6]
    const float *faces;              // [3][FACES] thresholds (positive cellsize only)
    uint32_t *bitmaps;               // [leaf hash][BITWORDS] occupancy of the leaf grids (bit = cell)
    uint32_t *seg_count;             // [leaf hash][RANK_SEGS] occupied cells per bitmap slice (accumulated by K1's flush)
    unsigned long long *hash_keys;   // [4 x leaf grids] leaf -> id: open addressing on the packed coordinates ...
    uint32_t *hash_ids;              //   ... and the id + 1 of the entry's leaf (0: not published yet, ~0: no grid left)
};

// Ranges of growing length (r4, the fast accumulate kernel's workgroups: they then reach their flush one after the other instead of
// all at once): range b has base_q + b * inc_q 1024ths of a step (256 points); this is the first step of range b.  Shared by the
// accumulate kernel, the replay kernel (which reads a range again when its box does not settle the octree's growth) and the host.
inline CWIPC_HOST_DEVICE uint32_t range_first_step(uint32_t b, uint32_t base_q, uint32_t inc_q) {
    const unsigned long long bb = b;
    return (uint32_t)((bb * base_q + (unsigned long long)inc_q * (bb * (bb > 0 ? bb - 1 : 0) / 2)) >> 10);
}

inline CWIPC_HOST_DEVICE uint64_t mix64(uint64_t k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

#if defined(__HIPCC__)
__device__ __forceinline__ unsigned long long pack_leaf(int lx, int ly, int lz) {
    return (1ull << 63) | ((unsigned long long)(uint32_t)(lx & 0x1fffff)) | ((unsigned long long)(uint32_t)(ly & 0x1fffff) << 21) |
           ((unsigned long long)(uint32_t)(lz & 0x1fffff) << 42);
}
__device__ __forceinline__ int unpack_leaf(unsigned long long v, int axis) {
    int t = (int)((v >> (21 * axis)) & 0x1fffff);
    return (t << 11) >> 11;   // sign-extend 21 bits
}

// ---------------------------------------------------------------------------
// global side: leaf lookup, record updates
// ---------------------------------------------------------------------------
// One lane: returns the id (hash position) of leaf key k, inserting it if new.
// The id (= grid) of leaf k, giving it the next free one if the pass has not met it yet; ~0 when the grids have run out
// (ERR_LEAVES is set: the host regrows and reruns).  The hash has four slots per grid: with one slot per grid (round 1: the
// slot WAS the id) a person-sized cloud's 12-16 leaves filled a 16-slot table and every lookup walked it, one global round
// trip per probe -- 5-10 us in the flush of every workgroup (time stamps of the debug-knob build).  Whoever claims a slot
// publishes the id right behind the claim; a lane that finds the key but not yet the id looks again in the SAME loop (no
// inner wait: lanes of one wave may be on either side).
__device__ __forceinline__ uint32_t leaf_lookup(const VoxWork &W, uint32_t mask, unsigned long long k) {
    const uint32_t cap = (mask + 1u) >> 2;
    uint32_t pos = (uint32_t)mix64(k) & mask;
    uint32_t probes = 0;
    for (uint32_t guard = 0; guard < (1u << 22); guard++) {
        unsigned long long cur = __hip_atomic_load(&W.hash_keys[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) {
            cur = atomicCAS(&W.hash_keys[pos], 0ull, k);
            if (cur == 0ull) {
                const uint32_t id = atomicAdd(&W.ctrl[C_LEAVES], 1u);
                if (id < cap) {
                    W.leaf_keys[id] = k;
                    __hip_atomic_store(&W.hash_ids[pos], id + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return id;
                }
                atomicOr(&W.ctrl[C_ERR], ERR_LEAVES);
                __hip_atomic_store(&W.hash_ids[pos], 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return 0xffffffffu;
            }
        }
        if (cur == k) {
            const uint32_t v = __hip_atomic_load(&W.hash_ids[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v != 0u) return v == 0xffffffffu ? 0xffffffffu : v - 1u;
            continue;   // claimed a moment ago, id on its way
        }
        pos = (pos + 1) & mask;
        if (++probes > mask) break;
    }
    atomicOr(&W.ctrl[C_ERR], ERR_LEAVES);
    return 0xffffffffu;
}

// The same question asked through the caches first (r4, second session; the fast accumulate kernel's flush).  An entry of the leaf table never
// changes once its id is published, and this XCD's L2 holds nothing older than the kernel's start: a plain load that shows the key WITH its id
// shows the truth, and one that does not (an empty slot, a key without its id, a line that went into L2 before the leaf was claimed) sends the lane
// to leaf_lookup's loads at device scope.  Those go past the L2 to the memory side, where the lookups of ALL workgroups -- a cloud has a dozen
// leaves, a 300 k-point cloud 234 workgroups that flush at the same moment -- queue at a dozen addresses: 1.2 to 13 us per lookup by the time stamps.
__device__ __forceinline__ uint32_t leaf_lookup_cached(const VoxWork &W, uint32_t mask, unsigned long long k) {
    uint32_t pos = (uint32_t)mix64(k) & mask;
    for (uint32_t probes = 0; probes < 8u; probes++) {
        const unsigned long long cur = __hip_atomic_load(&W.hash_keys[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (cur == k) {
            const uint32_t v = __hip_atomic_load(&W.hash_ids[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (v != 0u && v != 0xffffffffu) return v - 1u;
            break;
        }
        if (cur == 0ull) break;
        pos = (pos + 1) & mask;
    }
    return leaf_lookup(W, mask, k);
}

// Record of voxel key = leaf id << 19 | cell  (grids are CELLS records apart, not 2^19).
__device__ __forceinline__ unsigned long long *record_ptr(const VoxWork &W, uint32_t key) {
    return W.records + ((size_t)(key >> CELL_BITS) * CELLS + (key & ((1u << CELL_BITS) - 1))) * RECORD_WORDS;
}

// index into seg_count of the bitmap slice that holds a record's bit
__device__ __forceinline__ uint32_t slice_of(uint32_t key) {
    const uint32_t cell = key & ((1u << CELL_BITS) - 1);
    return (key >> CELL_BITS) * RANK_SEGS + (cell >> 5) / SEG_WORDS;
}

__device__ __forceinline__ void mark_occupied(const VoxWork &W, uint32_t key) {
    const uint32_t cell = key & ((1u << CELL_BITS) - 1);
    atomicOr(&W.bitmaps[(size_t)(key >> CELL_BITS) * BITWORDS + (cell >> 5)], 1u << (cell & 31u));
}

// Position inside the voxel as an integer: prod = fl(p * inv_leaf) is the number pcl::VoxelGrid floors, so
// prod - floor(prod) in [0, 1) is where the point sits in its voxel, in voxel units.  Adding 1.0 rounds that to a
// multiple of 2^-23 (ties to even, unbiased) and leaves it in the mantissa: q in [0, 2^23].  One v_fract and one add;
// the centroid is rebuilt as (voxel + sum q / (n 2^23)) / inv_leaf in f64 by the emit kernels (VoxParams::vox_unit, q_unit).
// Both accumulate kernels (the fast one and the general one) use this very function: their integer sums are identical.
constexpr uint32_t Q_ONE_BITS = 0x3f800000u;   // bits of 1.0f
__device__ __forceinline__ float voxel_fract(float prod) { return __builtin_amdgcn_fractf(prod); }
__device__ __forceinline__ uint32_t voxel_offset(float prod) { return __float_as_uint(__fadd_rn(voxel_fract(prod), 1.0f)) - Q_ONE_BITS; }
#endif   // __HIPCC__
}  // namespace
}  // namespace cwipc_amd
