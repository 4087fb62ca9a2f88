// voxel_k1_fast.inc -- the streaming pass of the voxel downsample, lean variant ("K1 fast").
// Included by kernels_voxel.hip inside namespace cwipc_amd { namespace { ... } }, after the shared definitions.
//
// Same job and same results as voxel_accumulate_kernel (the general variant, which stays as the fallback): one pass over
// the planes, per-voxel integer sums into the leaf grids.  Reference: pcl::VoxelGrid / OctreePointCloud as called by
// src/cwipc_filters.cpp:30-172 (restated in oracle/cwipc_oracle.c).  The general variant was bound by vector-instruction
// issue (706 VALU per 256-point wave step, profiles/r01); this one is written for instruction count:
//
//   * the key of a point in the workgroup's table is LINEAR in its voxel index: key = ix + (iy << 10) + (iz << 20)
//     (mod 2^32) -- two shift-adds per point, no leaf arithmetic, no base, no range test in the loop.  It is unique
//     while a workgroup's points span < 1024 x 1024 x 4096 voxels; the flush checks that span (from the waves' boxes) and
//     only then decodes keys into (leaf grid, cell).  Clouds that do not fit are handed to the general variant.
//     (Any 32-bit value is a key -- voxel (-1, 0, 0) is 0xffffffff -- so table entries carry 64-bit keys: the high word
//     holds the side bits below and is what tells an empty entry.)
//   * octree leaves (positive cellsize): a voxel belongs to two leaves only if a leaf face cuts it, and then the side
//     of a point is one bit per axis: s = [p >= T] for the face threshold T inside that voxel.  A wave keeps, per axis,
//     the one face its current step can meet (faces are 64 voxels apart) in scalar registers and classifies whole
//     steps with its lanes' minima and maxima: below the face, clear above the cut voxel, or mixed -- only mixed steps
//     (the few that touch a cut voxel) pay per-point compares.  The side bits are the high word of the table key.
//   * position inside the voxel: voxel_offset() (one v_fract, one packed add), summed as raw mantissas.
//   * merge across the whole wave, conflict-free inserts: a lane forms prefix sums of its four points once; an inclusive
//     scan over the wave (DPP row shifts + two row broadcasts) turns them into wave-wide prefixes; a run of equal keys, however
//     many lanes it spans, is inserted ONCE, by the lane where it ends, as the difference of two prefixes (the one at its
//     end, and the one at the end of the run before, fetched with one ds_bpermute from the lane a ballot / clz names).
//     Lanes of one insert instruction therefore never hit the same table entry: LDS atomics of several lanes on one
//     address serialise, which is what made lane-local inserts slow (115 us).  Round 0 inserts the run that ends at the
//     lane's first boundary; the rare further boundaries inside a lane (up to three) take rounds of their own.
//   * packed fp32 (v_pk_mul_f32 / v_pk_add_f32) where two coordinates take the same operation; v_cvt_flr_i32_f32.
//   * steps with absent (ragged end) or non-finite points take a masked copy of the same code.
//
// What it does not do: tables that overflow (sparse or unordered clouds), steps wider than two leaves, workgroups wider
// than the key: each sets ERR_FAST_PATH and the host reruns the pass with the general variant.
// Measured (MI355X, 9 998 244 points, profiles/r02_*): 57-59 us alone (general variant: 67), 479 VALU / 181 SALU / 42 LDS
// instructions per wave step (general: 706 / 239 / 35); stage by stage in profiles/r02_k1_stages.txt.

#ifdef CWIPC_DEBUG_KNOBS
// phase time stamps of two workgroups (debug-knob builds only; 100 MHz counter), read and logged by the host
__device__ unsigned long long g_fast_stamps[2][16];
__device__ unsigned long long g_fast_wave_done[K1_WAVES];   // workgroup 0: when each wave had done its steps
__device__ unsigned long long g_wg_times[1024][4];         // every workgroup: start, streaming done (thread 0's wave), all waves done, end
#define FAST_STAMP(i) do { if (threadIdx.x == 0) { const unsigned long long t_ = wall_clock64(); if (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2) g_fast_stamps[blockIdx.x ? 1 : 0][i] = t_; \
    if (blockIdx.x < 1024 && ((i) == 0 || (i) == 2 || (i) == 3 || (i) == 7)) g_wg_times[blockIdx.x][(i) == 0 ? 0 : (i) == 2 ? 1 : (i) == 3 ? 2 : 3] = t_; } } while (0)
#else
#define FAST_STAMP(i) do { } while (0)
#endif

constexpr int KEY_SPAN_X = 1024, KEY_SPAN_Y = 1024, KEY_SPAN_Z = 4096;
constexpr unsigned long long KEY64_EMPTY = ~0ull;
constexpr uint32_t Q_NEG_ONE_BITS = 0u - Q_ONE_BITS;

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct FastParams {
    uint32_t n, per_wg;   // per_wg: points of a workgroup's contiguous range (multiple of WAVE_STEP); its waves share it step by step
    uint32_t range_base_q, range_inc_q;   // != 0: ranges of growing length instead (range_first_step, voxel_common.hpp); per_wg is then the longest
    float inv_leaf;
    int ib0, ib1, ib2;
    int fb0, fb1, fb2;
    uint32_t leaf_mask, list_cap, want_list;
    uint32_t dbg;   // -DCWIPC_DEBUG_KNOBS builds only (CWIPC_FAST_DBG): 1 no table inserts, 2 no run merge, 4 loads and boxes only, 8 no flush
};

// The workgroup's table (LTAB entries, K1_WAVES waves), what goes with it and the flush's lists.  One workgroup per CU.
struct FastTable {
    unsigned long long key[LTAB];   // side bits << 32 | linear voxel key; KEY64_EMPTY = free
    uint32_t tile[LTAB];
    unsigned long long a[LTAB];   // sum qx
    unsigned long long b[LTAB];   // sum qy
    unsigned long long c[LTAB];   // sum qz | sum b << 40
    unsigned long long d[LTAB];   // count | sum r << 16 | sum g << 40
    uint32_t faces[FACE_TABLE_WORDS];
    uint32_t htag[HIST], hcnt[HIST];
    unsigned long long leaf_tab[LOCAL_LEAVES];
    uint32_t leaf_gid[LOCAL_LEAVES];
    alignas(16) float slab[K1_WAVES][12];   // per wave and axis: tlo, tmid, tv, thi (see fast_refit); 16-byte aligned: three ds_read_b128 per step
    int slab_j[K1_WAVES][4];      // ... and the table index of tlo (-1: none yet)
    int tmin[3], tmax[3];         // voxel index range of the workgroup's points
    uint32_t nfresh, fresh_base, nused, err;
    uint32_t next_step;           // the next step of the workgroup's range nobody has taken yet
    float wbox[K1_WAVES][6];      // the waves' boxes, reduced to the range's box before the flush
    alignas(16) uint32_t used[LTAB];   // flush: the entries in use (16-byte aligned: the LDS layout the profiles/ figures were taken with)
    uint32_t rec[LTAB];           // flush: leaf id << 19 | cell of the entry's record, ~0 = none
    uint32_t fresh[LTAB];         // records this workgroup touched first (plain grid: they are listed)
};

// ((iz << 10) + iy << 10) + ix in two v_lshl_add_u32 (the compiler's own choice is two shifts and a three-operand add)
__device__ __forceinline__ uint32_t linear_key(int ix, int iy, int iz) {
    uint32_t t, k;
    asm("v_lshl_add_u32 %0, %1, 10, %2" : "=v"(t) : "v"(iz), "v"(iy));
    asm("v_lshl_add_u32 %0, %1, 10, %2" : "=v"(k) : "v"(t), "v"(ix));
    return k;
}
__device__ __forceinline__ float min2f(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float max2f(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ int cvt_floor_i32(float v) {
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// 11 bits from a linear key: fold the upper fields down, multiply by a 24-bit odd constant (full-rate v_mul_u32_u24)
__device__ __forceinline__ uint32_t fast_hash(uint32_t key, uint32_t side) {
    static_assert(LTAB <= 2048 && (LTAB & (LTAB - 1)) == 0, "11 bits at most");
    const uint32_t t = key ^ (key >> 13) ^ (side << 7);
    return (__umul24(t, 0x9E3779u) >> 13) & (uint32_t)(LTAB - 1);
}

// The whole wave calls these (active = this lane has a run to add): the slot of `key` in the workgroup table, claimed if
// new.  In two halves, so that the round trip of the first compare-and-swap (which finds the slot nine times out of ten)
// lies behind the work between them; fast_find_end returns false for lanes that found no room (table full: this cloud is
// for the general variant).
__device__ __forceinline__ unsigned long long fast_find_begin(FastTable &L, uint32_t key, uint32_t side, bool active, uint32_t &slot) {
    slot = fast_hash(key, side);
    unsigned long long old = KEY64_EMPTY;
    if (active) old = atomicCAS(&L.key[slot], KEY64_EMPTY, u64_of(key, side));
    return old;
}
__device__ __forceinline__ bool fast_find_end(FastTable &L, uint32_t key, uint32_t side, bool active, unsigned long long old, uint32_t &slot, uint32_t &err) {
    const unsigned long long key64 = u64_of(key, side);
    bool pending = active && !(old == KEY64_EMPTY || old == key64);
#pragma unroll 1
    for (int probe = 1; probe < LTAB_PROBES; probe++) {
        if (__ballot(pending) == 0ull) break;
        if (pending) {
            slot = (slot + 1) & (LTAB - 1);
            old = atomicCAS(&L.key[slot], KEY64_EMPTY, key64);
            if (old == KEY64_EMPTY || old == key64) pending = false;
        }
    }
    if (__ballot(active && pending) != 0ull) err |= ERR_FAST_PATH;
    return active && !pending;
}
__device__ __forceinline__ bool fast_find(FastTable &L, uint32_t key, uint32_t side, bool active, uint32_t &slot, uint32_t &err) {
    const unsigned long long old = fast_find_begin(L, key, side, active, slot);
    return fast_find_end(L, key, side, active, old, slot, err);
}

// the colour / count part and the z sum of a run into its entry (x and y go on their own, as soon as they are known)
__device__ __forceinline__ void fast_add_rest(FastTable &L, uint32_t slot, bool ok, uint32_t qz, uint32_t cr, uint32_t gb, uint32_t tile) {
    if (ok) {
        atomicAdd(&L.c[slot], u64_of(qz, (gb & 0xffffu) << 8));                                      // | sum b << 40
        atomicAdd(&L.d[slot], u64_of(__builtin_amdgcn_alignbit(cr, cr, 16), (gb >> 16) << 8));      // count | sum r << 16 | sum g << 40
        if ((L.tile[slot] & tile) != tile) atomicOr(&L.tile[slot], tile);   // almost always there already: a read is cheaper (r4: the OR sent
        // unconditionally, without the look -- no round trip for the wave to wait for at the end of a step -- measured the same: 54.0-54.4 us)
    }
}

// Slot of leaf k in the workgroup's leaf table (LDS only), claimed if new; ~0 when the table is full.
__device__ __forceinline__ uint32_t fast_leaf_slot(FastTable &L, unsigned long long k) {
    uint32_t pos = (((uint32_t)k ^ (uint32_t)(k >> 21) ^ (uint32_t)(k >> 42)) * 0x9E3779B1u) >> 26;   // LOCAL_LEAVES = 2^6
    for (int probe = 0; probe < LOCAL_LEAVES; probe++) {
        unsigned long long cur = L.leaf_tab[pos];
        if (cur == 0ull) {
            cur = atomicCAS(&L.leaf_tab[pos], 0ull, k);
            if (cur == 0ull) cur = k;
        }
        if (cur == k) return pos;
        pos = (pos + 1) & (LOCAL_LEAVES - 1);
    }
    return 0xffffffffu;
}

// inclusive prefix sum over the 64 lanes: four DPP row shifts inside rows of 16, two row broadcasts across them
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);    // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);    // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);    // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);    // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2 and 3
    return v;
}

// One face per axis that a wave's step can meet: the step must lie in [tlo, thi) = [Tv(j), T(j + 2)), from above the voxel
// face j cuts up to face j + 2, so that the one cut voxel inside is that of face j + 1; tmid = T(j + 1) is that face's
// threshold, tv = Tv(j + 1) the lower bound of the voxel above the cut one.  Any step narrower than 63 voxels fits one.
// The slabs of a wave live in LDS (FastTable::slab), read at the start of every step: wave-uniform, but kept out of the
// scalar registers, which the loop is short of.
//
// Moves a wave's slabs to where its current step is: per axis the leaf of the step's lowest point and the leaf above it.
// Called by the whole wave with the lanes' extremes (lanes without a valid point: +inf / -inf); false: the step lies off
// the threshold table or is wider than a slab -- not for the fast variant.  Out of line on purpose: it runs a few times
// per wave, and inlined into the step its temporaries cost the hot loop 30 registers.
__device__ __attribute__((noinline)) bool fast_refit(FastTable *Lp, int wave, float mn0, float mn1, float mn2, float mx0, float mx1, float mx2, float inv,
                                                      int ib0, int ib1, int ib2, int fb0, int fb1, int fb2) {
    FastTable &L = *Lp;
    float lo[3] = {mn0, mn1, mn2}, hi[3] = {mx0, mx1, mx2};
    for (int sft = 32; sft > 0; sft >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], sft, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], sft, 64));
        }
    }
    if (!(lo[0] <= hi[0])) return true;   // a step without any valid point leaves everything as it is
    const int ib[3] = {ib0, ib1, ib2}, fb[3] = {fb0, fb1, fb2};
    bool bad = false;
#pragma unroll 1
    for (int a = 0; a < 3; a++) {
        const float *T = reinterpret_cast<const float *>(&L.faces[FT_T + a * FACES]);
        const float *TV = reinterpret_cast<const float *>(&L.faces[FT_TV + a * FACES]);
        const float lowest = lo[a], highest = hi[a];
        int i = L.slab_j[wave][a];
        if (i < 0) i = ((cvt_floor_i32(lowest * inv) - ib[a]) >> 6) - fb[a];
        i = max(0, min(i, FACES - 3));
        for (int it = 0; it < FACES && i > 0 && lowest < TV[i]; it++) i--;
        for (int it = 0; it < FACES && i < FACES - 3 && lowest >= TV[i + 1]; it++) i++;
        const float tlo = TV[i], tmid = T[i + 1], tv = TV[i + 1], thi = T[i + 2];
        if (!(lowest >= tlo && lowest < tv && highest < thi)) bad = true;
        if ((threadIdx.x & 63) == 0) {
            L.slab[wave][4 * a + 0] = tlo; L.slab[wave][4 * a + 1] = tmid; L.slab[wave][4 * a + 2] = tv; L.slab[wave][4 * a + 3] = thi;
            L.slab_j[wave][a] = i;
        }
    }
    return !bad;
}

// The leaf of the workgroup's first point, looked up in the global leaf table while the workgroup streams (r4, second session).  Every call
// starts with an empty leaf table, so in their flushes ALL workgroups of a cloud meet at its dozen leaves at once: the time stamps of a
// 300 k-point cloud's workgroups put the flush's one lookup per leaf between 1.2 and 13 us (whoever claims a leaf publishes its id a round
// trip or two later; everybody else polls), and a workgroup of such a cloud lives 10 to 26 us.  A workgroup's first point certainly counts
// and certainly lies in one of its leaves -- for a cloud in scan order: in the leaf most of its entries belong to --, so one lane of the
// last wave (where it has no step to take: small clouds) finds that leaf by the general
// kernel's rule (point_key_lookup: the two face thresholds around the voxel), claims its slot in the workgroup's leaf table and asks the
// global table right away; the flush asks only for leaves that have no id yet.  Out of line: it runs once per workgroup.
// (Everything by value: a pointer to the kernel's parameter blocks would put them into scratch memory for the whole kernel.)
template <int MODE>
__device__ __attribute__((noinline)) void fast_scout(FastTable *Lp, float inv_leaf, int ib0, int ib1, int ib2, int fb0, int fb1, int fb2, uint32_t leaf_mask,
                                                      unsigned long long *hash_keys, uint32_t *hash_ids, unsigned long long *leaf_keys, uint32_t *ctrl,
                                                      float f0, float f1, float f2) {
    FastTable &L = *Lp;
    const float f[3] = {f0, f1, f2};
    if (!__builtin_isfinite(f0 + f1 + f2)) return;
    const int ib[3] = {ib0, ib1, ib2}, fb[3] = {fb0, fb1, fb2};
    int l[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int t = cvt_floor_i32(__fmul_rn(f[a], inv_leaf)) - ib[a];
        if (MODE == 0) {
            l[a] = t >> 6;
        } else {
            const int m = (t + 32) >> 6;                          // the face nearest to this voxel
            const unsigned i = (unsigned)(m - fb[a]);
            if (!(i + 1u < (unsigned)FACES)) return;                // beyond the threshold table: the flush will say so
            const float *T = reinterpret_cast<const float *>(&L.faces[FT_T + a * FACES]);
            l[a] = m - 1 + (f[a] >= T[i] ? 1 : 0) + (f[a] >= T[i + 1] ? 1 : 0);
        }
        if (!(l[a] > -(1 << 20) && l[a] < (1 << 20))) return;
    }
    const unsigned long long k = pack_leaf(l[0], l[1], l[2]);
    const uint32_t ls = fast_leaf_slot(L, k);
    if (ls == 0xffffffffu) return;
    VoxWork w{};   // (what leaf_lookup reads of it)
    w.hash_keys = hash_keys; w.hash_ids = hash_ids; w.leaf_keys = leaf_keys; w.ctrl = ctrl;
    L.leaf_gid[ls] = leaf_lookup(w, leaf_mask, k);
}

// A wave's box: three minima and three maxima over the wave (DPP row shifts + two row broadcasts), valid in lane 63.  All six at once,
// one fused DPP instruction per value and stage: the five instructions between two stages of one value cover the two wait states a
// DPP read of a fresh result needs.  (Written as six calls of a scan with __builtin_amdgcn_update_dpp the compiler made
// v_mov / s_nop / v_mov_dpp / v_min / s_nop of every stage: 189 instructions with 65 s_nop at the end of every wave's range,
// in front of the flush's first barrier -- a wave issues one instruction per ~4.7 cycles: 0.35 us; now 37.)
__device__ __forceinline__ void wave_box_to_63(float &n0, float &n1, float &n2, float &x0, float &x1, float &x2) {
#define CWIPC_BOX_STAGE(CTRL)                                \
    "v_min_f32_dpp %0, %0, %0 " CTRL "\n"                    \
    "v_min_f32_dpp %1, %1, %1 " CTRL "\n"                    \
    "v_min_f32_dpp %2, %2, %2 " CTRL "\n"                    \
    "v_max_f32_dpp %3, %3, %3 " CTRL "\n"                    \
    "v_max_f32_dpp %4, %4, %4 " CTRL "\n"                    \
    "v_max_f32_dpp %5, %5, %5 " CTRL "\n"
    asm volatile("s_nop 1\n"
                 CWIPC_BOX_STAGE("row_shr:1 row_mask:0xf bank_mask:0xf")
                 CWIPC_BOX_STAGE("row_shr:2 row_mask:0xf bank_mask:0xf")
                 CWIPC_BOX_STAGE("row_shr:4 row_mask:0xf bank_mask:0xf")
                 CWIPC_BOX_STAGE("row_shr:8 row_mask:0xf bank_mask:0xf")
                 CWIPC_BOX_STAGE("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 CWIPC_BOX_STAGE("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 : "+v"(n0), "+v"(n1), "+v"(n2), "+v"(x0), "+v"(x1), "+v"(x2));
#undef CWIPC_BOX_STAGE
}

// The end of a workgroup's pass: every wave hands in its error bits and the box of the points it has seen; then the table is
// flushed into the leaf grids' records (see the kernel's header).  Errors that the general accumulate kernel does not have set
// ERR_FAST_PATH: the host then reruns the pass with that kernel.
// Returns false when nothing of this workgroup may reach the records (an error has been recorded: the whole workgroup leaves).
// A workgroup may flush more than once (round 4: its range in two sub-ranges): the boxes are those of everything its waves have
// seen so far -- what the octree replay wants of the last flush, and a superset of the keys' span for the earlier ones -- and the
// leaf table with its ids stays from flush to flush.
//
// Round 3: this tail was 4 to 13.5 us per workgroup (8.5 in the middle; per-workgroup time stamps, 10 M points), and NOT because
// of its atomics -- without any of them it still took 5.4 us for the record loop alone: eight fixed, fully unrolled rounds of a
// loop whose body was a switch over the record's eight words, every case run by every wave, each behind its own chain of LDS reads.
// Now: entries are decoded in the pass that compacts them (one barrier less); the occupancy bits are requested one entry per
// lane, all at once, ahead of the record updates; a lane knows from the start which two table words and which shifts make ITS
// word of the record (no switch), and the update loop runs as many rounds as there are entries.
// Part 1 of the end of a workgroup's pass: errors, the range's box (out to W.bboxes), the voxel span of its points.
// Returns 0: the range held no point that counts (nothing to flush); 1: go on, tmn = the lowest voxel index per axis (the base of
// the linear keys); 2: an error has been recorded, nothing of this workgroup may reach the records.
__device__ __forceinline__ int fast_finish_head(FastTable &L, const FastParams &P, const VoxWork &W, uint32_t err, float bn0, float bn1, float bn2, float bx0, float bx1,
                                                float bx2, int &tmn0, int &tmn1, int &tmn2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv = P.inv_leaf;
    // ---- errors of this wave, bounding box of its range (input of the octree replay), extent in voxels ----
    if (__ballot(err != 0u) != 0ull) {
        for (int s = 32; s > 0; s >>= 1) err |= (uint32_t)__shfl_xor((int)err, s, 64);
        if (lane == 0) atomicOr(&L.err, err);
    }
    {
        float vlo0 = bn0, vlo1 = bn1, vlo2 = bn2, vhi0 = bx0, vhi1 = bx1, vhi2 = bx2;
        wave_box_to_63(vlo0, vlo1, vlo2, vhi0, vhi1, vhi2);
        if (lane == 63) {
            L.wbox[wave][0] = vlo0; L.wbox[wave][1] = vlo1; L.wbox[wave][2] = vlo2;
            L.wbox[wave][3] = vhi0; L.wbox[wave][4] = vhi1; L.wbox[wave][5] = vhi2;
            if (vlo0 <= vhi0) {
                atomicMin(&L.tmin[0], cvt_floor_i32(vlo0 * inv)); atomicMin(&L.tmin[1], cvt_floor_i32(vlo1 * inv)); atomicMin(&L.tmin[2], cvt_floor_i32(vlo2 * inv));
                atomicMax(&L.tmax[0], cvt_floor_i32(vhi0 * inv)); atomicMax(&L.tmax[1], cvt_floor_i32(vhi1 * inv)); atomicMax(&L.tmax[2], cvt_floor_i32(vhi2 * inv));
            }
        }
    }
    tmn0 = tmn1 = tmn2 = 0;
#ifdef CWIPC_DEBUG_KNOBS
    if (P.dbg & 8u) return 0;
#endif
    __syncthreads();
    FAST_STAMP(3);
    if (threadIdx.x < 6) {   // the range's box (input of the octree replay): the waves' boxes reduced
        float v = L.wbox[0][threadIdx.x];
        for (int w = 1; w < K1_WAVES; w++) v = threadIdx.x < 3 ? fminf(v, L.wbox[w][threadIdx.x]) : fmaxf(v, L.wbox[w][threadIdx.x]);
        W.bboxes[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
    tmn0 = L.tmin[0]; tmn1 = L.tmin[1]; tmn2 = L.tmin[2];
    const bool any_points = tmn0 <= L.tmax[0];
    uint32_t wg_err = L.err;
    if (any_points) {
        // the linear keys are unique only inside this span; also keep indices where int arithmetic on them is safe
        const long long span0 = (long long)L.tmax[0] - tmn0, span1 = (long long)L.tmax[1] - tmn1, span2 = (long long)L.tmax[2] - tmn2;
        if (span0 >= KEY_SPAN_X - 1 || span1 >= KEY_SPAN_Y - 1 || span2 >= KEY_SPAN_Z - 1) wg_err |= ERR_FAST_PATH;
        const int big = 1 << 28;
        if (tmn0 < -big || tmn1 < -big || tmn2 < -big || L.tmax[0] > big || L.tmax[1] > big || L.tmax[2] > big) wg_err |= ERR_RANGE;
    }
    if (wg_err) {
        // nothing of this workgroup reaches the records: the host discards the pass and runs another one
        if (threadIdx.x == 0) atomicOr(&W.ctrl[C_ERR], wg_err);
        return 2;
    }
    return any_points ? 1 : 0;
}

// Part 2: the table's entries (linear keys relative to tmn) -> the leaf grids' records, first touches counted.
template <int MODE>
__device__ __forceinline__ void fast_flush_records(FastTable &L, const FastParams &P, const VoxWork &W, const int tmn0, const int tmn1, const int tmn2) {
    constexpr int UU = 2;   // entries a group of eight lanes has in flight in the record loop
    const int lane = threadIdx.x & 63;
    const uint32_t key_base = (uint32_t)((((tmn2 << 10) + tmn1) << 10) + tmn0);
    // ---- the entries in use: decoded to (local leaf slot << 19 | cell) and compacted in one pass ----
    // (every lane runs the arithmetic, whatever its entry holds; only entries in use claim a leaf slot and a place in the lists:
    // one LDS atomic per wave for the places, not per entry -- many lanes on one counter serialise)
    uint32_t bad = 0;
    constexpr int PER_THREAD = (LTAB + K1_THREADS - 1) / K1_THREADS;
    unsigned long long kk[PER_THREAD];
#pragma unroll
    for (int q = 0; q < PER_THREAD; q++) {
        const int e = (int)threadIdx.x + q * K1_THREADS;
        kk[q] = e < LTAB ? L.key[e] : KEY64_EMPTY;
    }
#pragma unroll
    for (int q = 0; q < PER_THREAD; q++) {
        const int e = (int)threadIdx.x + q * K1_THREADS;
        const unsigned long long k64 = kk[q];
        const bool in_use = k64 != KEY64_EMPTY;
        const uint32_t dk = (uint32_t)k64 - key_base, side = (uint32_t)(k64 >> 32);
        const int t[3] = {tmn0 + (int)(dk & 1023u), tmn1 + (int)((dk >> 10) & 1023u), tmn2 + (int)(dk >> 20)};
        const int ib[3] = {P.ib0, P.ib1, P.ib2}, fb[3] = {P.fb0, P.fb1, P.fb2};
        int leaf[3], cell[3];
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (MODE == 0) {
                leaf[a] = (t[a] - ib[a]) >> 6;
            } else {
                // leaf of the voxel's lower part: l with tf(l) < t <= tf(l + 1); plus the side bit.  tf(l) is ib + 64 l give
                // or take a voxel, so the estimate is off by one at most: the four table words around it decide (read side by
                // side, not one after the other)
                const int *TF = reinterpret_cast<const int *>(&L.faces[FT_TF + a * FACES]);
                int j = ((t[a] - ib[a] - 1) >> 6) - fb[a];
                j = max(1, min(j, FACES - 3));
                const int fm = TF[j - 1], f0 = TF[j], f1 = TF[j + 1], f2 = TF[j + 2];
                const int d = t[a] <= f0 ? -1 : (t[a] > f1 ? 1 : 0);
                const int flo = d < 0 ? fm : d > 0 ? f1 : f0, fhi = d < 0 ? f0 : d > 0 ? f2 : f1;
                j += d;
                ok &= flo < t[a] && t[a] <= fhi;
                leaf[a] = fb[a] + j + (int)((side >> a) & 1u);
            }
            cell[a] = t[a] - ib[a] - 64 * leaf[a] + 2;
            ok &= (unsigned)cell[a] < (unsigned)GRID_DIM;
            ok &= leaf[a] > -(1 << 20) && leaf[a] < (1 << 20);
        }
        // (the leaf by its slot in the workgroup's leaf table for now: the global ids are fetched once per leaf and
        // workgroup below -- every lane asking the global table itself means 150 k requests for a dozen addresses at the
        // same moment, measured 20 us)
        uint32_t rec = 0xffffffffu;
        if (in_use) {
            if (ok) {
                const uint32_t ls = fast_leaf_slot(L, pack_leaf(leaf[0], leaf[1], leaf[2]));
                if (ls != 0xffffffffu) rec = (ls << CELL_BITS) | (uint32_t)((cell[2] * GRID_DIM + cell[1]) * GRID_DIM + cell[0]);
                else bad |= ERR_FAST_PATH;   // more than 64 leaves in one workgroup
            } else {
                bad |= ERR_CELL_RANGE;
            }
        }
        const unsigned long long vote = __ballot(in_use);
        uint32_t base = 0;
        if (lane == 0 && vote != 0ull) base = atomicAdd(&L.nused, (uint32_t)__popcll(vote));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (in_use) {
            const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(vote >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)vote, 0u));
            L.used[at] = (uint32_t)e;
            L.rec[at] = rec;
        }
    }
    if (__ballot(bad != 0u) != 0ull) {
        for (int sft = 32; sft > 0; sft >>= 1) bad |= (uint32_t)__shfl_xor((int)bad, sft, 64);
        if (lane == 0) atomicOr(&W.ctrl[C_ERR], bad);
    }
    __syncthreads();
    FAST_STAMP(5);
    const uint32_t nused = L.nused;
#ifdef CWIPC_DEBUG_KNOBS
    if (P.dbg & 512u) return;   // after compaction and decode, before the leaf ids
#endif
    // one request per leaf and workgroup to the global leaf table (~0: it is full, ERR_LEAVES is set, the host regrows and reruns)
    if (threadIdx.x < LOCAL_LEAVES) {
        const unsigned long long lk = L.leaf_tab[threadIdx.x];
#ifdef CWIPC_DEBUG_KNOBS
        if (P.dbg & 256u) { if (lk != 0ull) L.leaf_gid[threadIdx.x] = threadIdx.x; } else
#endif
        if (lk != 0ull && L.leaf_gid[threadIdx.x] == 0xffffffffu) L.leaf_gid[threadIdx.x] = leaf_lookup_cached(W, P.leaf_mask, lk);   // (fast_scout has one of them already)
    }
    __syncthreads();
    FAST_STAMP(6);
#ifdef CWIPC_DEBUG_KNOBS
    if (P.dbg & 128u) return;   // after the leaf ids
#endif
    // ---- occupancy bits: one entry per lane, all requested before the record updates go out (this is the serial tail of the
    // kernel; a loop that waits for each occupancy word costs a memory round trip per iteration: measured 17 us for the flush) ----
    uint32_t okey[PER_THREAD], oold[PER_THREAD];
#pragma unroll
    for (int q = 0; q < PER_THREAD; q++) {
        const uint32_t i = threadIdx.x + (uint32_t)q * K1_THREADS;
        okey[q] = 0xffffffffu; oold[q] = 0xffffffffu;
        if (i >= nused) continue;
        const uint32_t ks = L.rec[i];
        if (ks == 0xffffffffu) continue;
        const uint32_t gid = L.leaf_gid[ks >> CELL_BITS];
        if (gid == 0xffffffffu) continue;
        const uint32_t cell = ks & ((1u << CELL_BITS) - 1);
        okey[q] = (gid << CELL_BITS) | cell;
#ifdef CWIPC_DEBUG_KNOBS
        if (P.dbg & 32u) oold[q] = 0; else
#endif
        oold[q] = atomicOr(&W.bitmaps[(size_t)gid * BITWORDS + (cell >> 5)], 1u << (cell & 31u));
    }
    // ---- record updates: eight lanes per entry, lane `sub` adds word `sub` of the 64-byte record (fire and forget) ----
    // word 0: sum qx (table word a); 1: sum qy (b); 2: sum qz (c, low 40 bits); 3: count << 32 | sum r (d: count | r << 16);
    // 4: sum g << 32 | sum b (d >> 40, c >> 40); 5, 6: tile bits 0-3 / 4-7 as 16-bit contribution counters; 7: nothing.
    // Every lane reads two table words and takes (w1 >> s1) & m1 as the low half, (w2 >> s2) & m2 as the high half.
    {
        const int sub = lane & 7;
        const int f1 = sub == 0 ? 0 : sub == 1 ? 1 : sub == 2 ? 2 : sub == 3 ? 3 : 2;          // a, b, c, d, c
        const int f2 = sub == 0 ? 0 : sub == 1 ? 1 : sub == 2 ? 2 : 3;                         // a, b, c, d, d
        const uint32_t s1 = sub == 3 ? 16u : sub == 4 ? 40u : 0u, s2 = sub == 3 ? 0u : sub == 4 ? 40u : 32u;
        const uint32_t m1 = (sub == 3 || sub == 4) ? 0xffffffu : 0xffffffffu;
        const uint32_t m2 = sub == 2 ? 0xffu : sub == 3 ? 0xffffu : sub == 4 ? 0xffffffu : 0xffffffffu;
        const bool tile_word = sub == 5 || sub == 6;
        const unsigned long long *const w1p = f1 == 0 ? L.a : f1 == 1 ? L.b : f1 == 2 ? L.c : L.d, *const w2p = f2 == 0 ? L.a : f2 == 1 ? L.b : f2 == 2 ? L.c : L.d;
        for (uint32_t i0 = threadIdx.x >> 3; i0 < nused; i0 += UU * (K1_THREADS / 8)) {
            uint32_t e[UU], ks[UU];
#pragma unroll
            for (int u = 0; u < UU; u++) {
                const uint32_t i = i0 + (uint32_t)u * (K1_THREADS / 8);
                e[u] = L.used[i < nused ? i : i0];
                ks[u] = i < nused ? L.rec[i] : 0xffffffffu;
            }
            uint32_t gid[UU], tl[UU];
            unsigned long long w1[UU], w2[UU];
#pragma unroll
            for (int u = 0; u < UU; u++) {
                gid[u] = L.leaf_gid[ks[u] != 0xffffffffu ? ks[u] >> CELL_BITS : 0u];
                if (ks[u] == 0xffffffffu) gid[u] = 0xffffffffu;
                w1[u] = w1p[e[u]]; w2[u] = w2p[e[u]];
                tl[u] = L.tile[e[u]] >> (sub == 6 ? 4 : 0);
            }
#pragma unroll
            for (int u = 0; u < UU; u++) {
                if (gid[u] == 0xffffffffu) continue;
                uint32_t vlo = (uint32_t)(w1[u] >> s1) & m1, vhi = (uint32_t)(w2[u] >> s2) & m2;
                if (tile_word) {
                    vlo = (tl[u] & 1u) | ((tl[u] & 2u) << 15);
                    vhi = ((tl[u] >> 2) & 1u) | ((tl[u] & 8u) << 13);
                }
#ifdef CWIPC_DEBUG_KNOBS
                if (!(P.dbg & 16u))
#endif
                // (no result wanted; nothing to add -- the word of the tile bits 4-7 of a cloud whose cameras are 1, 2, 4, 8 -- is not sent:
                // what bounds the flushes, all of them at the same time, is the rate at which the memory side retires atomics)
                if (sub < 7 && (vlo | vhi) != 0u) atomicAdd(&record_ptr(W, (gid[u] << CELL_BITS) | (ks[u] & ((1u << CELL_BITS) - 1)))[sub], u64_of(vlo, vhi));
            }
        }
    }
    // ---- whoever set a record's occupancy bit has touched the record first: counted per bitmap slice, listed for the plain grid ----
#pragma unroll
    for (int q = 0; q < PER_THREAD; q++) {
        const uint32_t k = okey[q];
        const bool fresh = k != 0xffffffffu && !(oold[q] & (1u << (k & 31u)));
        const unsigned long long fv = __ballot(fresh);
        if (fv == 0ull) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&L.nfresh, (uint32_t)__popcll(fv));   // (one LDS atomic per wave)
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (fresh) {
            if (P.want_list) L.fresh[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(fv >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fv, 0u))] = k;
            const uint32_t sl = slice_of(k);
            uint32_t hs = (sl * 0x9E3779B1u) >> 24;   // HIST = 2^8
            bool counted = false;
            for (int probe = 0; probe < 8 && !counted; probe++) {
                const uint32_t tag = atomicCAS(&L.htag[hs], 0u, sl + 1u);
                if (tag == 0u || tag == sl + 1u) {
                    atomicAdd(&L.hcnt[hs], 1u);
                    counted = true;
                }
                hs = (hs + 1) & (HIST - 1);
            }
            if (!counted) atomicAdd(&W.seg_count[sl], 1u);
        }
    }
    __syncthreads();
    FAST_STAMP(7);
    if (threadIdx.x < HIST && L.htag[threadIdx.x]) atomicAdd(&W.seg_count[L.htag[threadIdx.x] - 1u], L.hcnt[threadIdx.x]);
    const uint32_t nfresh = L.nfresh;
    if (threadIdx.x == 0) atomicMax(&W.ctrl[C_MAXLOAD], nused);
    if (!P.want_list) {
        if (threadIdx.x == 0 && nfresh) atomicAdd(&W.ctrl[C_COUNT], nfresh);
        return;
    }
    if (threadIdx.x == 0 && nfresh) L.fresh_base = atomicAdd(&W.ctrl[C_COUNT], nfresh);
    __syncthreads();
    FAST_STAMP(8);
    for (uint32_t i = threadIdx.x; i < nfresh; i += K1_THREADS) {
        const uint32_t idx = L.fresh_base + i;
        if (idx < P.list_cap) W.occupied[idx] = L.fresh[i];
        else atomicOr(&W.ctrl[C_ERR], ERR_LIST_FULL);
    }
}

template <int MODE>
__device__ __forceinline__ void fast_finish(FastTable &L, const FastParams &P, const VoxWork &W, uint32_t err, float bn0, float bn1, float bn2, float bx0, float bx1,
                                            float bx2) {
    int tmn0, tmn1, tmn2;
    if (fast_finish_head(L, P, W, err, bn0, bn1, bn2, bx0, bx1, bx2, tmn0, tmn1, tmn2) != 1) return;
    fast_flush_records<MODE>(L, P, W, tmn0, tmn1, tmn2);
}

// MODE 0: plain grid (bricks of 64 voxels on the voxel lattice), 1: octree leaves by face thresholds.
// K1_THREADS threads and an LTAB-entry table per workgroup: one workgroup per CU.
//
// Round 4, measured and removed again (commit 78186d1 has the code): two workgroups of 8 waves and 1024 entries per CU
// (profiles/r04_k1_pair_experiment.txt); the table left in the workspace for a merge kernel to take to the records
// (profiles/r04_k1_dump_merge.txt); the staggered ranges in reverse order (profiles/r04_k1_stagger.txt).
//
// Round 4, measured and NOT kept (commit bbddfb3 has the code, profiles/r04_k1_pair_experiment.txt the figures): two workgroups of
// 8 waves per CU, each taking its range as two sub-ranges with a flush after each -- a third and two thirds for the one, two
// thirds and a third for the other, told apart by the base of their LDS allocation (HW_REG_LDS_ALLOC) -- so that one of a CU's
// two streams while the other flushes.  Bit-identical; 61.8 us against 53.3-54.0 on the same box (two workgroups per CU with one
// flush each: 55.1-56.0).  A range's table holds about as many entries whether the range is 13 scan lines or 4 (a scan line of
// this cloud meets ~190 voxels and the lines of a range meet the same ones): four flushes per CU are 1.5 x the records and four
// times the barriers and round trips of one, and the eight waves that stream meanwhile have half the loads in flight.
template <int MODE>
__global__ void __launch_bounds__(K1_THREADS, 4) voxel_accumulate_fast_kernel(FastParams P, const float *__restrict__ x, const float *__restrict__ y,
                                                                             const float *__restrict__ z, const uint32_t *__restrict__ rgbt, VoxWork W) {
    extern __shared__ __align__(16) unsigned char k1_smem[];
    FastTable &L = *reinterpret_cast<FastTable *>(k1_smem);
    FAST_STAMP(0);

    const int lane = threadIdx.x & 63;
    // The workgroup owns a contiguous range of the planes; its waves take the range's steps (256 points) one by one from a
    // counter in LDS instead of owning a sixteenth each: the SIMD serves its four waves oldest first, so with fixed shares the
    // first waves were done after 23 us and the last ones ran alone, one wave per SIMD, until 40 us (time stamps of the
    // debug-knob build); sharing keeps four waves per SIMD busy to the end.
    const int wave = threadIdx.x >> 6;
    uint32_t chunk_lo = blockIdx.x * P.per_wg, chunk_hi = min(chunk_lo + P.per_wg, P.n);
    if (P.range_base_q != 0u) {
        chunk_lo = min(range_first_step(blockIdx.x, P.range_base_q, P.range_inc_q) * (uint32_t)WAVE_STEP, P.n);
        chunk_hi = min(range_first_step(blockIdx.x + 1u, P.range_base_q, P.range_inc_q) * (uint32_t)WAVE_STEP, P.n);
    }
    const int chunk_pts = chunk_lo < chunk_hi ? (int)(chunk_hi - chunk_lo) : 0;
    const int nsteps = (chunk_pts + WAVE_STEP - 1) / WAVE_STEP;
    // one step's 64 bytes per lane: the step's base address is wave-uniform (scalar registers), the lane adds its 16 bytes
    auto load_step = [&](int step, float4 &ax, float4 &ay, float4 &az, uint4 &aw) __attribute__((always_inline)) {
        const size_t at = (size_t)chunk_lo + (size_t)(uint32_t)__builtin_amdgcn_readfirstlane(step) * WAVE_STEP;
        ax = reinterpret_cast<const float4 *>(x + at)[lane];
        ay = reinterpret_cast<const float4 *>(y + at)[lane];
        az = reinterpret_cast<const float4 *>(z + at)[lane];
        aw = reinterpret_cast<const uint4 *>(rgbt + at)[lane];
    };
    // the first step (wave w: step w) is loaded before the table is initialised (planes are padded to whole steps)
    float4 cx = make_float4(0, 0, 0, 0), cy = cx, cz = cx;
    uint4 cw = make_uint4(0, 0, 0, 0);
    int cur = wave < nsteps ? wave : -1;
#ifdef CWIPC_DEBUG_KNOBS
    // timing experiment: only 12 / 8 of the 16 waves take steps (the others help with the flush): how much does the streaming
    // phase owe to the waves that hide each other's waits?
    const int streamers = (P.dbg & 0x20000u) ? 8 : (P.dbg & 0x10000u) ? 12 : K1_WAVES;
    if (wave >= streamers) cur = -1;
#else
    constexpr int streamers = K1_WAVES;
#endif
    if (cur >= 0) load_step(cur, cx, cy, cz, cw);

    // (the threshold table's words are requested before the table is cleared and stored behind it: their round trip lies
    // behind the clearing)
    constexpr int FT_PER_LANE = (FACE_TABLE_WORDS + K1_THREADS - 1) / K1_THREADS;
    uint32_t ftw[FT_PER_LANE];
    if (MODE == 1) {
        const uint32_t *ft = reinterpret_cast<const uint32_t *>(W.faces);
#pragma unroll
        for (int q = 0; q < FT_PER_LANE; q++) ftw[q] = (int)threadIdx.x + q * K1_THREADS < FACE_TABLE_WORDS ? ft[threadIdx.x + q * K1_THREADS] : 0u;
    }
    auto clear_table = [&]() __attribute__((always_inline)) {
        for (int i = threadIdx.x; i < LTAB; i += K1_THREADS) {
            L.key[i] = KEY64_EMPTY; L.tile[i] = 0;
            L.a[i] = 0; L.b[i] = 0; L.c[i] = 0; L.d[i] = 0;
        }
        if (threadIdx.x < HIST) { L.htag[threadIdx.x] = 0; L.hcnt[threadIdx.x] = 0; }
        if (threadIdx.x == 0) { L.nfresh = 0; L.nused = 0; }
    };
    clear_table();
    if (MODE == 1) {
#pragma unroll
        for (int q = 0; q < FT_PER_LANE; q++)
            if ((int)threadIdx.x + q * K1_THREADS < FACE_TABLE_WORDS) L.faces[threadIdx.x + q * K1_THREADS] = ftw[q];
    }
    if (threadIdx.x < LOCAL_LEAVES) { L.leaf_tab[threadIdx.x] = 0ull; L.leaf_gid[threadIdx.x] = 0xffffffffu; }
    if (threadIdx.x < 3) { L.tmin[threadIdx.x] = INT32_MAX; L.tmax[threadIdx.x] = INT32_MIN; }
    if (threadIdx.x < K1_WAVES * 12) (&L.slab[0][0])[threadIdx.x] = INFINITY;   // cover nothing yet: the first step sets the slabs
    if (threadIdx.x < K1_WAVES * 4) (&L.slab_j[0][0])[threadIdx.x] = -1;
    if (threadIdx.x == 0) { L.err = 0; L.next_step = (uint32_t)streamers; }
    __syncthreads();
    FAST_STAMP(1);
    // (only where the last wave has no step of its own -- clouds up to a million points: 100 k points 23.7 -> 22.0 us, 300 k 26.1 -> 24.3, 1 M 31.0 -> 30.2;
    // with every wave streaming, 10 M points, the lookups of all workgroups at the kernel's start cost 0.5 us more than they save in the staggered flushes)
    // (ONE scout per workgroup: every wave without a step scouting a point of its own, spread over the range, so that the range's second and third leaf are
    // there too, made the kernel slower -- 100 k points 23.6 -> 28.6-31.5 us, 300 k 26 -> 29: eleven lookups per workgroup at the kernel's start are the crowd
    // at the leaf table over again.)
    if (wave == K1_WAVES - 1 && lane == 0 && chunk_pts > 0 && nsteps < K1_WAVES)
        fast_scout<MODE>(&L, P.inv_leaf, P.ib0, P.ib1, P.ib2, P.fb0, P.fb1, P.fb2, P.leaf_mask, W.hash_keys, W.hash_ids, W.leaf_keys, W.ctrl, x[chunk_lo], y[chunk_lo], z[chunk_lo]);

    const float inv = P.inv_leaf;
    const f32x2 inv2 = {inv, inv};
    const f32x2 one2 = {1.0f, 1.0f};
    float bn0 = FLT_MAX, bn1 = FLT_MAX, bn2 = FLT_MAX, bx0 = -FLT_MAX, bx1 = -FLT_MAX, bx2 = -FLT_MAX;
    uint32_t err = 0;
    // One step = this lane's four consecutive points, in cx / cy / cz / cw.  MASKED: some point of the wave's step is absent
    // or not finite.  The step is ordered so that few registers are alive at a time (128 per lane, 16 of them hold the next
    // step's loads, and a spill reload would wait for every load in flight): everything that needs the coordinates first,
    // then the colour words, and only then the run merge, one field at a time.
    auto step = [&](auto masked_tag, const float4 cx, const float4 cy, const float4 cz, const uint4 cw, int left) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        bool v0 = true, v1 = true, v2 = true, v3 = true;
        if (MASKED) {
            // as the octree does (addPointsFromInputCloud: isFinite); one test per point: the sum is NaN or Inf iff a
            // coordinate is (or they are beyond any sane range)
            v0 = left > 0 && __builtin_isfinite(cx.x + cy.x + cz.x);
            v1 = left > 1 && __builtin_isfinite(cx.y + cy.y + cz.y);
            v2 = left > 2 && __builtin_isfinite(cx.z + cy.z + cz.z);
            v3 = left > 3 && __builtin_isfinite(cx.w + cy.w + cz.w);
        }
        // ---- the lane's extremes: range box of the wave (input of the octree replay), slab tests ----
        float mn0, mn1, mn2, mx0, mx1, mx2;
        if (!MASKED) {
            // (all twelve are numbers here: plain v_min / v_max, where fminf / fmaxf would have the compiler quiet every operand first)
            mn0 = min3f(cx.x, cx.y, min2f(cx.z, cx.w)); mx0 = max3f(cx.x, cx.y, max2f(cx.z, cx.w));
            mn1 = min3f(cy.x, cy.y, min2f(cy.z, cy.w)); mx1 = max3f(cy.x, cy.y, max2f(cy.z, cy.w));
            mn2 = min3f(cz.x, cz.y, min2f(cz.z, cz.w)); mx2 = max3f(cz.x, cz.y, max2f(cz.z, cz.w));
        } else {
            const float pinf = INFINITY, ninf = -INFINITY;
            auto lo4 = [&](float a, float b, float c, float d) { return fminf(fminf(v0 ? a : pinf, v1 ? b : pinf), fminf(v2 ? c : pinf, v3 ? d : pinf)); };
            auto hi4 = [&](float a, float b, float c, float d) { return fmaxf(fmaxf(v0 ? a : ninf, v1 ? b : ninf), fmaxf(v2 ? c : ninf, v3 ? d : ninf)); };
            mn0 = lo4(cx.x, cx.y, cx.z, cx.w); mx0 = hi4(cx.x, cx.y, cx.z, cx.w);
            mn1 = lo4(cy.x, cy.y, cy.z, cy.w); mx1 = hi4(cy.x, cy.y, cy.z, cy.w);
            mn2 = lo4(cz.x, cz.y, cz.z, cz.w); mx2 = hi4(cz.x, cz.y, cz.z, cz.w);
        }
        // (updated in place: written as r = min3(r, v, v) the compiler gave every result a new register and moved it back at the end of
        // the step -- six of the step's 303 vector instructions)
        asm("v_min3_f32 %0, %0, %1, %1" : "+v"(bn0) : "v"(mn0)); asm("v_max3_f32 %0, %0, %1, %1" : "+v"(bx0) : "v"(mx0));
        asm("v_min3_f32 %0, %0, %1, %1" : "+v"(bn1) : "v"(mn1)); asm("v_max3_f32 %0, %0, %1, %1" : "+v"(bx1) : "v"(mx1));
        asm("v_min3_f32 %0, %0, %1, %1" : "+v"(bn2) : "v"(mn2)); asm("v_max3_f32 %0, %0, %1, %1" : "+v"(bx2) : "v"(mx2));

#ifdef CWIPC_DEBUG_KNOBS
        if (P.dbg & 4u) { bn0 = fminf(bn0, __uint_as_float(cw.x ^ cw.y ^ cw.z ^ cw.w)); return; }
#endif
        uint32_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;   // side bits (octree): bit a = the point lies above the leaf face that cuts its voxel on axis a
        bool sided = false;                        // wave-uniform: some point of this step may have a side bit
        bool dead = false;                         // wave-uniform: the step cannot be taken (an error has been recorded)
        float4 sl0, sl1, sl2;
        if (MODE == 1) {
            // is the step inside the wave's slabs?  (lanes without a valid point carry +-inf and pass)
            const float4 *sl = reinterpret_cast<const float4 *>(&L.slab[wave][0]);
            sl0 = sl[0]; sl1 = sl[1]; sl2 = sl[2];   // x = tlo, y = tmid, z = tv, w = thi
            const bool inside = (mn0 >= sl0.x) & (mx0 < sl0.w) & (mn1 >= sl1.x) & (mx1 < sl1.w) & (mn2 >= sl2.x) & (mx2 < sl2.w);
            if (__builtin_expect(__ballot(!inside) != 0ull, 0)) {
                if (!fast_refit(&L, wave, mn0, mn1, mn2, mx0, mx1, mx2, inv, P.ib0, P.ib1, P.ib2, P.fb0, P.fb1, P.fb2)) { err |= ERR_FAST_PATH; dead = true; }
                sl0 = sl[0]; sl1 = sl[1]; sl2 = sl[2];
            }
            // Which side of the face?  Only points inside the voxel the face cuts need a bit: steps below the face or
            // clear above that voxel have none.
            // (r4: ONE ballot on the common path -- does any lane's span reach into [tmid, tv) on any axis? -- where rounds 2 and 3 took six,
            // "all lanes below the face" and "all lanes clear above the cut voxel" per axis: a lane whose own minimum and maximum do not
            // bracket that interval has no point in it.  Lanes without a valid point carry +inf / -inf and never qualify.)
            const bool t0 = (mx0 >= sl0.y) & (mn0 < sl0.z), t1 = (mx1 >= sl1.y) & (mn1 < sl1.z), t2 = (mx2 >= sl2.y) & (mn2 < sl2.z);
            if (__builtin_expect(__ballot(t0 | t1 | t2) != 0ull, 0)) {
                sided = true;
                if (__ballot(t0) != 0ull) {
                    h0 |= (cx.x >= sl0.y && cx.x < sl0.z) ? 1u : 0u; h1 |= (cx.y >= sl0.y && cx.y < sl0.z) ? 1u : 0u;
                    h2 |= (cx.z >= sl0.y && cx.z < sl0.z) ? 1u : 0u; h3 |= (cx.w >= sl0.y && cx.w < sl0.z) ? 1u : 0u;
                }
                if (__ballot(t1) != 0ull) {
                    h0 |= (cy.x >= sl1.y && cy.x < sl1.z) ? 2u : 0u; h1 |= (cy.y >= sl1.y && cy.y < sl1.z) ? 2u : 0u;
                    h2 |= (cy.z >= sl1.y && cy.z < sl1.z) ? 2u : 0u; h3 |= (cy.w >= sl1.y && cy.w < sl1.z) ? 2u : 0u;
                }
                if (__ballot(t2) != 0ull) {
                    h0 |= (cz.x >= sl2.y && cz.x < sl2.z) ? 4u : 0u; h1 |= (cz.y >= sl2.y && cz.y < sl2.z) ? 4u : 0u;
                    h2 |= (cz.z >= sl2.y && cz.z < sl2.z) ? 4u : 0u; h3 |= (cz.w >= sl2.y && cz.w < sl2.z) ? 4u : 0u;
                }
            }
        }

        // ---- voxel index and position inside the voxel: fl(p * inv_leaf), floor, fract (+ 1: raw mantissas) ----
        uint32_t k0, k1, k2, k3;
        uint32_t rx0, rx1, rx2, rx3, ry0, ry1, ry2, ry3, rz0, rz1, rz2, rz3;
        {
            const f32x2 qx01 = f32x2{cx.x, cx.y} * inv2, qx23 = f32x2{cx.z, cx.w} * inv2;
            const f32x2 qy01 = f32x2{cy.x, cy.y} * inv2, qy23 = f32x2{cy.z, cy.w} * inv2;
            const f32x2 qz01 = f32x2{cz.x, cz.y} * inv2, qz23 = f32x2{cz.z, cz.w} * inv2;
            const int ix0 = cvt_floor_i32(qx01.x), ix1 = cvt_floor_i32(qx01.y), ix2 = cvt_floor_i32(qx23.x), ix3 = cvt_floor_i32(qx23.y);
            const int iy0 = cvt_floor_i32(qy01.x), iy1 = cvt_floor_i32(qy01.y), iy2 = cvt_floor_i32(qy23.x), iy3 = cvt_floor_i32(qy23.y);
            const int iz0 = cvt_floor_i32(qz01.x), iz1 = cvt_floor_i32(qz01.y), iz2 = cvt_floor_i32(qz23.x), iz3 = cvt_floor_i32(qz23.y);
            // keys: linear in the voxel index
            k0 = linear_key(ix0, iy0, iz0); k1 = linear_key(ix1, iy1, iz1);
            k2 = linear_key(ix2, iy2, iz2); k3 = linear_key(ix3, iy3, iz3);
            const f32x2 fx01 = f32x2{voxel_fract(qx01.x), voxel_fract(qx01.y)} + one2, fx23 = f32x2{voxel_fract(qx23.x), voxel_fract(qx23.y)} + one2;
            const f32x2 fy01 = f32x2{voxel_fract(qy01.x), voxel_fract(qy01.y)} + one2, fy23 = f32x2{voxel_fract(qy23.x), voxel_fract(qy23.y)} + one2;
            const f32x2 fz01 = f32x2{voxel_fract(qz01.x), voxel_fract(qz01.y)} + one2, fz23 = f32x2{voxel_fract(qz23.x), voxel_fract(qz23.y)} + one2;
            rx0 = __float_as_uint(fx01.x); rx1 = __float_as_uint(fx01.y); rx2 = __float_as_uint(fx23.x); rx3 = __float_as_uint(fx23.y);
            ry0 = __float_as_uint(fy01.x); ry1 = __float_as_uint(fy01.y); ry2 = __float_as_uint(fy23.x); ry3 = __float_as_uint(fy23.y);
            rz0 = __float_as_uint(fz01.x); rz1 = __float_as_uint(fz01.y); rz2 = __float_as_uint(fz23.x); rz3 = __float_as_uint(fz23.y);
        }
        // ---- colours, count, tiles ----
        PointAdd a0 = point_add(cw.x), a1 = point_add(cw.y), a2 = point_add(cw.z), a3 = point_add(cw.w);
        // one camera per wave step almost always (then every run has that tile)
        const uint32_t tile_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)a0.tile);
        const uint32_t tiles4 = __builtin_amdgcn_perm(__builtin_amdgcn_perm(cw.w, cw.z, 0x0c0c0703u), __builtin_amdgcn_perm(cw.y, cw.x, 0x0c0c0703u), 0x05040100u);
        const bool one_tile = !MASKED && __ballot(tiles4 != tile_u * 0x01010101u) == 0ull;
        if (MASKED) {
            // a point that does not count joins the run of a neighbour and adds nothing to it
            const uint32_t kv = v0 ? k0 : v1 ? k1 : v2 ? k2 : k3, hv = v0 ? h0 : v1 ? h1 : v2 ? h2 : h3;
            k0 = v0 ? k0 : kv; k1 = v1 ? k1 : k0; k2 = v2 ? k2 : k1; k3 = v3 ? k3 : k2;
            h0 = v0 ? h0 : hv; h1 = v1 ? h1 : h0; h2 = v2 ? h2 : h1; h3 = v3 ? h3 : h2;
            auto drop = [](bool v, uint32_t &rx, uint32_t &ry, uint32_t &rz, PointAdd &a) {
                if (!v) { rx = ry = rz = Q_ONE_BITS; a.cr = 0; a.gb = 0; }
            };
            drop(v0, rx0, ry0, rz0, a0); drop(v1, rx1, ry1, rz1, a1); drop(v2, rx2, ry2, rz2, a2); drop(v3, rx3, ry3, rz3, a3);
        }
        const uint32_t C1 = a0.cr, C2 = C1 + a1.cr, C3 = C2 + a2.cr, C4 = C3 + a3.cr;
        const uint32_t G1 = a0.gb, G2 = G1 + a1.gb, G3 = G2 + a2.gb, G4 = G3 + a3.gb;
        // the tiles of the four points (needed only where cameras meet); a point that does not count has its neighbour's
        uint32_t u0 = tiles4 & 0xffu, u1 = (tiles4 >> 8) & 0xffu, u2 = (tiles4 >> 16) & 0xffu, u3 = tiles4 >> 24;
        if (MASKED) {
            const uint32_t uv = v0 ? u0 : v1 ? u1 : v2 ? u2 : u3;
            u0 = v0 ? u0 : uv; u1 = v1 ? u1 : u0; u2 = v2 ? u2 : u1; u3 = v3 ? u3 : u2;
        }
        const uint32_t tiles = u0 | (u1 << 8) | (u2 << 16) | (u3 << 24);
        const uint32_t hp = h0 | (h1 << 3) | (h2 << 6) | (h3 << 9);   // (all zero unless `sided`)

        // prefix sums over the lane's points; the exponent bits go as the sums are formed (v_add3_u32)
        const uint32_t X1 = rx0 + Q_NEG_ONE_BITS, X2 = X1 + rx1 + Q_NEG_ONE_BITS, X3 = X2 + rx2 + Q_NEG_ONE_BITS, X4 = X3 + rx3 + Q_NEG_ONE_BITS;
        const uint32_t Y1 = ry0 + Q_NEG_ONE_BITS, Y2 = Y1 + ry1 + Q_NEG_ONE_BITS, Y3 = Y2 + ry2 + Q_NEG_ONE_BITS, Y4 = Y3 + ry3 + Q_NEG_ONE_BITS;
        const uint32_t Z1 = rz0 + Q_NEG_ONE_BITS, Z2 = Z1 + rz1 + Q_NEG_ONE_BITS, Z3 = Z2 + rz2 + Q_NEG_ONE_BITS, Z4 = Z3 + rz3 + Q_NEG_ONE_BITS;

        // ---- runs: one table insert per run, by the lane where the run ends ----
        // A run of equal keys may span several lanes; its sum is the difference of two prefix sums over the wave's 256
        // points: at its end, and at the end of the run before it.  Every lane knows the prefix at each of its own
        // boundaries (wave-exclusive prefix of the lane totals + prefix inside the lane); the prefix at the previous
        // boundary comes from the same lane, or from the nearest lower lane that has one (ds_bpermute).  So a run is
        // inserted once, by one lane, and no two lanes of an insert round touch the same table entry: LDS atomics on
        // one address serialise (lane-local inserts, measured: 115 us for the kernel).
#ifdef CWIPC_DEBUG_KNOBS
        if (P.dbg & 2u) { bx0 = fmaxf(bx0, __uint_as_float((X4 ^ Y4 ^ Z4 ^ C4 ^ G4 ^ k0 ^ k1 ^ k2 ^ k3 ^ hp ^ tiles) & 0x3fffffffu)); return; }
#endif
        const uint32_t kn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)k0, 0x130, 0xf, 0xf, true);   // wave_shl:1: the next lane's first key
        bool b1 = k1 != k0, b2 = k2 != k1, b3 = k3 != k2, b4 = (k3 != kn) | (lane == 63);
        if (__builtin_expect(sided, 0)) {
            const uint32_t hn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hp, 0x130, 0xf, 0xf, true) & 7u;
            const uint32_t hx = hp ^ (hp >> 3);
            b1 |= (hx & 7u) != 0u; b2 |= (hx & 0x38u) != 0u; b3 |= (hx & 0x1c0u) != 0u; b4 |= (hp >> 9) != hn;
        }
        if (__builtin_expect(!one_tile, 0)) {
            // where cameras meet, a change of tile ends a run too, and a run's tile is that of its last point
            const uint32_t un = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tiles, 0x130, 0xf, 0xf, true) & 0xffu;
            const uint32_t tx = tiles ^ (tiles >> 8);
            b1 |= (tx & 0xffu) != 0u; b2 |= (tx & 0xff00u) != 0u; b3 |= (tx & 0xff0000u) != 0u; b4 |= (tiles >> 24) != un;
        }
        const uint32_t bits = (b1 ? 1u : 0u) | (b2 ? 2u : 0u) | (b3 ? 4u : 0u) | (b4 ? 8u : 0u);
        // the nearest lower lane with a boundary (none: the run started with the step, prefix 0)
        const unsigned long long has = __ballot(bits != 0u);
        const uint32_t lt_lo = lane >= 32 ? 0xffffffffu : (1u << lane) - 1u, lt_hi = lane > 32 ? (1u << (lane - 32)) - 1u : 0u;   // lanes below this one
        const uint32_t below_lo = (uint32_t)has & lt_lo, below_hi = (uint32_t)(has >> 32) & lt_hi;
        const bool none_below = (below_lo | below_hi) == 0u;
        const int prev_lane = below_hi ? 63 - __clz((int)below_hi) : 31 - __clz((int)below_lo);   // (garbage if none_below: masked below)
        const int paddr = prev_lane << 2;
        auto tile_at = [&](uint32_t j) { return one_tile ? tile_u : ((tiles >> (8u * j)) & 0xffu); };   // tile of point j (0..3)
        auto side_at = [&](uint32_t j) { return sided ? ((hp >> (3u * j)) & 7u) : 0u; };
        // One field at a time (and the scheduler is told to keep it so; five at once need more registers than a lane has):
        // E = wave-exclusive prefix of the lane totals (DPP scan); E + A[last boundary] is published for the lanes above;
        // Q = what the nearest lane below with a boundary published = where this lane's lowest run starts.  Returns the sum
        // of the lane's LOWEST run: E + A[first boundary] - Q.  The lane's other runs lie inside it: differences of the A's.
        auto field = [&](uint32_t A1, uint32_t A2, uint32_t A3, uint32_t A4) {
            const uint32_t E = wave_inclusive_scan(A4) - A4;
            const uint32_t Lf = E + (b4 ? A4 : b3 ? A3 : b2 ? A2 : A1);
            const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute(paddr, (int)Lf);
            const uint32_t first = b1 ? A1 : b2 ? A2 : b3 ? A3 : A4;
            return E + first - (none_below ? 0u : got);
        };
#ifdef CWIPC_DEBUG_KNOBS
        if (P.dbg & 1u) {
            const uint32_t t = field(C1, C2, C3, C4) ^ field(X1, X2, X3, X4) ^ field(Y1, Y2, Y3, Y4) ^ field(Z1, Z2, Z3, Z4) ^ field(G1, G2, G3, G4);
            bx1 = fmaxf(bx1, __uint_as_float(t & 0x3fffffffu));
            return;
        }
#endif
        if (!dead) {
            // round 0: the run that ends at the lane's FIRST boundary (most lanes have one boundary or none)
            const uint32_t j0 = b1 ? 0u : b2 ? 1u : b3 ? 2u : 3u;   // the point it ends with
            // (the fields in two groups, and the scheduler is told to keep them apart: five at once need more registers than
            // a lane has; the slot search's first round trip lies behind the first group)
            const uint32_t key0 = b1 ? k0 : b2 ? k1 : b3 ? k2 : k3, side0 = side_at(j0);
            uint32_t slot;
            unsigned long long found = KEY64_EMPTY;
            if (!MASKED) found = fast_find_begin(L, key0, side0, bits != 0u, slot);
            const uint32_t cnt0 = field(C1, C2, C3, C4);
            const uint32_t sx0 = field(X1, X2, X3, X4);
            const uint32_t sy0 = field(Y1, Y2, Y3, Y4);
            __builtin_amdgcn_sched_barrier(0);
            // (masked steps: a run of points that do not count must not claim an entry, so the count comes first)
            const bool act0 = bits != 0u && (!MASKED || (cnt0 >> 16) != 0u);
            if (MASKED) found = fast_find_begin(L, key0, side0, act0, slot);
            const bool ok0 = fast_find_end(L, key0, side0, act0, found, slot, err);
            if (ok0) {
                atomicAdd(&L.a[slot], u64_of(sx0, 0u));
                atomicAdd(&L.b[slot], u64_of(sy0, 0u));
            }
            const uint32_t sz0 = field(Z1, Z2, Z3, Z4);
            const uint32_t sg0 = field(G1, G2, G3, G4);
            __builtin_amdgcn_sched_barrier(0);
            fast_add_rest(L, slot, ok0, sz0, cnt0, sg0, tile_at(j0));
            // rounds 1..3: the lane's further boundaries, upwards; their runs start at the boundary below, in the same lane.
            // (Some lane has one in four steps out of five.  Parking these runs in a queue of the wave in LDS and inserting them a
            // full wave at a time -- a wave parks about twenty in its ten steps: one dense insert before the flush -- was built in
            // round 3: bit-identical, 53.2-53.9 us against 53.0-53.4, and 32 KB of LDS more: not kept.)
            uint32_t left_bits = bits & (bits - 1u);   // the first one is done
            if (__builtin_expect(__ballot(left_bits != 0u) != 0ull, 0)) {
                // prefix at the boundary below (starts as the first boundary's)
                uint32_t BX = b1 ? X1 : b2 ? X2 : X3, BY = b1 ? Y1 : b2 ? Y2 : Y3, BZ = b1 ? Z1 : b2 ? Z2 : Z3, BC = b1 ? C1 : b2 ? C2 : C3, BG = b1 ? G1 : b2 ? G2 : G3;
#pragma unroll 1
                for (int round = 1; round < 4; round++) {
                    const bool mine = left_bits != 0u;
                    // this round's boundary: after point 2, 3 or 4 (bit 1, 2 or 3)
                    const bool at2 = (left_bits & 2u) != 0u, at3 = !at2 && (left_bits & 4u) != 0u;
                    const uint32_t TX = at2 ? X2 : at3 ? X3 : X4, TY = at2 ? Y2 : at3 ? Y3 : Y4, TZ = at2 ? Z2 : at3 ? Z3 : Z4;
                    const uint32_t TC = at2 ? C2 : at3 ? C3 : C4, TG = at2 ? G2 : at3 ? G3 : G4;
                    const uint32_t j = at2 ? 1u : at3 ? 2u : 3u;
                    const uint32_t cnt = TC - BC;
                    const bool ok = fast_find(L, at2 ? k1 : at3 ? k2 : k3, side_at(j), mine && (!MASKED || (cnt >> 16) != 0u), slot, err);
                    if (ok) {
                        atomicAdd(&L.a[slot], u64_of(TX - BX, 0u));
                        atomicAdd(&L.b[slot], u64_of(TY - BY, 0u));
                    }
                    fast_add_rest(L, slot, ok, TZ - BZ, cnt, TG - BG, tile_at(j));
                    BX = TX; BY = TY; BZ = TZ; BC = TC; BG = TG;
                    left_bits &= left_bits - 1u;
                    if (__ballot(left_bits != 0u) == 0ull) break;
                }
            }
        }
    };

    auto grab = [&]() -> int {   // the next step nobody has taken, -1 when the range is exhausted (wave-uniform)
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&L.next_step, 1u);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        return t < (uint32_t)nsteps ? (int)t : -1;
    };
    int nxt = cur >= 0 ? grab() : -1;
#pragma unroll 1
    while (cur >= 0) {
        cur = __builtin_amdgcn_readfirstlane(cur);   // (wave-uniform by construction: keep them in scalar registers)
        nxt = __builtin_amdgcn_readfirstlane(nxt);
        // keep the next step's 64 bytes per lane in flight while this step is processed
        float4 nx = cx, ny = cy, nz = cz;
        uint4 nw = cw;
        if (nxt >= 0) load_step(nxt, nx, ny, nz, nw);
        const int left = chunk_pts - cur * WAVE_STEP - lane * 4;   // points of this lane that exist: min(left, 4)
        // anything absent or not finite in this step?  (packed adds: a sum is NaN or Inf iff one of its terms is, or
        // they are beyond any sane range -- the masked copy looks at every point)
        const f32x2 sx = f32x2{cx.x, cx.y} + f32x2{cx.z, cx.w}, sy = f32x2{cy.x, cy.y} + f32x2{cy.z, cy.w}, sz = f32x2{cz.x, cz.y} + f32x2{cz.z, cz.w};
        const f32x2 sa = (sx + sy) + sz;
        const bool odd = left < 4 || !__builtin_isfinite(sa.x + sa.y);
        if (__builtin_expect(__ballot(odd) == 0ull, 1)) step(std::false_type{}, cx, cy, cz, cw, left);
        else step(std::true_type{}, cx, cy, cz, cw, left);
        cx = nx; cy = ny; cz = nz; cw = nw;
        cur = nxt;
        if (cur >= 0) nxt = grab();
    }

    FAST_STAMP(2);   // (thread 0's wave: end of its own steps)
#ifdef CWIPC_DEBUG_KNOBS
    if (blockIdx.x == 0 && lane == 0 && wave < K1_WAVES) g_fast_wave_done[wave] = wall_clock64();
#endif
    fast_finish<MODE>(L, P, W, err, bn0, bn1, bn2, bx0, bx1, bx2);
}
