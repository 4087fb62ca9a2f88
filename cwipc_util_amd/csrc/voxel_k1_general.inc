// voxel_k1_general.inc -- the general accumulate kernel of the voxel-grid downsample (included by kernels_voxel.hip): leaf by
// threshold compare, DPP segmented scan over chains of lanes, overflow path to the global records.  It takes every cloud, and is
// what the fast variant (voxel_k1_fast.inc) hands a cloud back to (ERR_FAST_PATH).

// ---------------------------------------------------------------------------
// K1
// ---------------------------------------------------------------------------
// K1 is bound by instruction issue, not by HBM (rocprofv3: ~230 VALU instructions per point in the
// first version, VALU busy 60 %, waves parked 58 % with 4 waves per SIMD), so the hot loop below is
// written for instruction count: wave-uniform values in SGPRs, selects instead of branches, 32-bit
// arithmetic, byte permutes for the colour sums, and slow paths behind wave-uniform ballots.

// One run of points of the same voxel, 32-bit in-wave form (at most 256 points).
struct Run32 {
    uint32_t key;       // leaf id << 19 | cell, KEY_EMPTY = none
    uint32_t qx, qy, qz;   // sums of biased fixed-point offsets inside the voxel
    uint32_t cr;        // count << 16 | sum r
    uint32_t gb;        // sum g << 16 | sum b
    uint32_t tile;
};

// Workgroup table entry, 4 packed 64-bit sums.  A workgroup sees fewer than 65536 points, so
// count < 2^16, colour sums < 2^24, and a biased offset sum < 2^40.
struct LdsTable {
    uint32_t key[LTAB];
    uint32_t tile[LTAB];
    unsigned long long a[LTAB];   // sum (qx + bias)
    unsigned long long b[LTAB];   // sum (qy + bias)
    unsigned long long c[LTAB];   // sum (qz + bias) | sum b << 40
    unsigned long long d[LTAB];   // count | sum r << 16 | sum g << 40
    uint32_t fresh[LTAB];         // records this workgroup touched first
    float faces[3 * FACES];
    uint32_t htag[HIST], hcnt[HIST];  // first touches per bitmap slice of this workgroup (slice + 1, count); linear probing
    uint32_t nfresh, fresh_base;
    uint32_t nfallback, nused;    // table-full fallbacks of this workgroup; entries in use (counted by the flush)
    unsigned long long leaf_tab[LOCAL_LEAVES];   // packed leaf coordinates, 0 = free; position = local leaf slot
    uint32_t leaf_gid[LOCAL_LEAVES];             // global leaf id of each slot (filled before the flush)
    uint32_t nn_leaf[K1_WAVES][64];              // per wave: leaf (slot or id) of each leaf position relative to the cached faces, ~0 = not looked up yet
};

// The slim parameter block of K1 (kernel arguments live in SGPRs; K1 is short of them).
struct K1Params {
    uint32_t n, per_wave;
    float inv_leaf;
    int ib0, ib1, ib2;
    int fb0, fb1, fb2;
    uint32_t leaf_mask, list_cap, ablate;
    uint32_t local_leaves;   // 1: keys carry workgroup-local leaf slots (no global memory access in the hot loop)
    uint32_t want_list;      // 1: the touched records are listed in W.occupied (plain grid: the sort needs them); 0: only counted
    double mn0[3];      // MODE 2 only
    double res;
};

__device__ __forceinline__ unsigned long long u64_of(uint32_t lo, uint32_t hi) { return ((unsigned long long)hi << 32) | lo; }

// Add one run to the workgroup table.  All in-wave sums are 32-bit (<= 256 points), so the four
// packed 64-bit addends are assembled from 32-bit halves.
// One lane: slot of leaf k in the workgroup's local leaf table, inserting it if new; 0xffffffff when the table is full.
__device__ __forceinline__ uint32_t local_leaf_slot(LdsTable &L, unsigned long long k) {
    uint32_t pos = (((uint32_t)k ^ (uint32_t)(k >> 21) ^ (uint32_t)(k >> 42)) * 0x9E3779B1u) >> 26;   // LOCAL_LEAVES = 2^6
    for (int probe = 0; probe < LOCAL_LEAVES; probe++) {
        const unsigned long long cur = L.leaf_tab[pos];
        if (cur == k) return pos;
        if (cur == 0ull) {
            const unsigned long long old = atomicCAS(&L.leaf_tab[pos], 0ull, k);
            if (old == 0ull || old == k) return pos;
        }
        pos = (pos + 1) & (LOCAL_LEAVES - 1);
    }
    return 0xffffffffu;
}

// One lane: leaf k as the hot loop names it (a local slot, or the global id).  Whoever creates a local
// slot also fetches its global id right away, while the other waves keep streaming: the flush at the end
// of the kernel is a serial tail and should not start with a round trip to the global leaf table.
__device__ __forceinline__ uint32_t leaf_name(LdsTable &L, const VoxWork &W, const K1Params &P, unsigned long long k) {
    if (!P.local_leaves) return leaf_lookup(W, P.leaf_mask, k);
    const uint32_t slot = local_leaf_slot(L, k);
    if (slot != 0xffffffffu && atomicCAS(&L.leaf_gid[slot], 0xffffffffu, 0xfffffffeu) == 0xffffffffu) {
        L.leaf_gid[slot] = leaf_lookup(W, P.leaf_mask, k);   // ~0 if the global table is full (ERR_LEAVES is set then)
    }
    return slot;
}

__device__ __forceinline__ void lds_insert(LdsTable &L, const VoxWork &W, const K1Params &P, const Run32 &r, bool active) {
    // Called by the whole wave (active = this lane has something to insert).  The slot search is a loop
    // of its own, so that the adds are issued once per call however many probes the unluckiest lane needs:
    // LDS atomics are the scarcest resource of this kernel.
    uint32_t slot = (r.key * 0x9E3779B1u) >> (32 - 11);   // LTAB = 2^11
    bool pending = active;
#pragma unroll 1
    for (int probe = 0; probe < LTAB_PROBES; probe++) {
        if (pending) {
            const uint32_t old = atomicCAS(&L.key[slot], KEY_EMPTY, r.key);
            if (old == KEY_EMPTY || old == r.key) pending = false;
            else slot = (slot + 1) & (LTAB - 1);
        }
        if (__ballot(pending) == 0ull) break;
    }
    if (active && !pending) {
        // every offset carries its bias already, so the in-wave sums are plain unsigned 32-bit numbers
        atomicAdd(&L.a[slot], u64_of(r.qx, 0u));
        atomicAdd(&L.b[slot], u64_of(r.qy, 0u));
        atomicAdd(&L.c[slot], u64_of(r.qz, (r.gb & 0xffffu) << 8));                                            // | sum b << 40
        atomicAdd(&L.d[slot], u64_of(__builtin_amdgcn_alignbit(r.cr, r.cr, 16), (r.gb >> 16) << 8));         // count | sum r << 16 | sum g << 40
    }
    // the tile bits of a voxel are almost always there already: a plain read is much cheaper than an atomic
    const bool need_or = active && !pending && (L.tile[slot] & r.tile) != r.tile;
    if (__ballot(need_or) != 0ull) {
        if (need_or) atomicOr(&L.tile[slot], r.tile);
    }
    // ---- table saturated (sparse or incoherent input): the runs go straight to the global records ----
    const unsigned long long failed = __ballot(active && pending);
    if (__builtin_expect(failed != 0ull, 0)) {
        const bool mine = active && pending;
        const int lane = threadIdx.x & 63;
        // the record of this lane's run (global leaf id * CELLS + cell), ~0 if it has none
        uint32_t rec = 0xffffffffu;
        if (mine) {
            atomicAdd(&L.nfallback, 1u);
            uint32_t gid = r.key >> CELL_BITS;
            if (P.local_leaves) {
                gid = L.leaf_gid[r.key >> CELL_BITS];
                if (gid >= 0xfffffffeu) gid = leaf_lookup(W, P.leaf_mask, L.leaf_tab[r.key >> CELL_BITS]);   // ~0: ERR_LEAVES is set, the pass is discarded
            }
            if (gid != 0xffffffffu) rec = gid * (uint32_t)CELLS + (r.key & ((1u << CELL_BITS) - 1));
        }
        // Eight lanes per run update its 64-byte record with one instruction (one cache-line operation
        // in L2 instead of six: incoherent clouds are bound by exactly that), eight runs per instruction.
#pragma unroll 1
        for (int b = 0; b < 8; b++) {
            if (((failed >> (8 * b)) & 0xffull) == 0ull) continue;
            const int src = 8 * b + (lane >> 3), sub = lane & 7;
            const uint32_t s_rec = (uint32_t)__shfl((int)rec, src, 64);
            const uint32_t s_qx = (uint32_t)__shfl((int)r.qx, src, 64), s_qy = (uint32_t)__shfl((int)r.qy, src, 64), s_qz = (uint32_t)__shfl((int)r.qz, src, 64);
            const uint32_t s_cr = (uint32_t)__shfl((int)r.cr, src, 64), s_gb = (uint32_t)__shfl((int)r.gb, src, 64), s_tile = (uint32_t)__shfl((int)r.tile, src, 64);
            bool first = false;
            uint32_t s_key = 0;
            if (s_rec != 0xffffffffu && sub < 7) {
                const uint32_t cnt = s_cr >> 16;
                unsigned long long val;
                switch (sub) {
                case 0: val = s_qx; break;
                case 1: val = s_qy; break;
                case 2: val = s_qz; break;
                case 3: val = u64_of(s_cr & 0xffffu, cnt); break;                 // count << 32 | sum r
                case 4: val = u64_of(s_gb & 0xffffu, s_gb >> 16); break;         // sum g << 32 | sum b
                case 5:   // tile bits 0-3 as 16-bit contribution counters
                    val = (unsigned long long)(s_tile & 1u) | ((unsigned long long)((s_tile >> 1) & 1u) << 16) |
                          ((unsigned long long)((s_tile >> 2) & 1u) << 32) | ((unsigned long long)((s_tile >> 3) & 1u) << 48);
                    break;
                default:  // tile bits 4-7
                    val = (unsigned long long)((s_tile >> 4) & 1u) | ((unsigned long long)((s_tile >> 5) & 1u) << 16) |
                          ((unsigned long long)((s_tile >> 6) & 1u) << 32) | ((unsigned long long)((s_tile >> 7) & 1u) << 48);
                    break;
                }
                const unsigned long long old = atomicAdd(&W.records[(size_t)s_rec * RECORD_WORDS + sub], val);
                if (sub == 3 && (old >> 32) == 0) {
                    first = true;
                    s_key = ((s_rec / (uint32_t)CELLS) << CELL_BITS) | (s_rec % (uint32_t)CELLS);
                    mark_occupied(W, s_key);
                    atomicAdd(&W.seg_count[slice_of(s_key)], 1u);
                }
            }
            // records touched for the first time: counted (and listed) with one atomic per instruction
            const unsigned long long news = __ballot(first);
            if (news != 0ull) {
                const uint32_t nnew = (uint32_t)__popcll(news);
                uint32_t base = 0;
                if (lane == __ffsll((long long)news) - 1) base = atomicAdd(&W.ctrl[C_COUNT], nnew);
                if (P.want_list) {
                    base = (uint32_t)__shfl((int)base, __ffsll((long long)news) - 1, 64);
                    if (first) {
                        const uint32_t idx = base + (uint32_t)__popcll(news & ((1ull << lane) - 1ull));
                        if (idx < P.list_cap) W.occupied[idx] = s_key;
                        else atomicOr(&W.ctrl[C_ERR], ERR_LIST_FULL);
                    }
                }
            }
        }
    }
}

// DPP row shifts inside rows of 16 lanes (lanes whose source is outside the row read 0).
template <int N>
__device__ __forceinline__ int dpp_shr(int v) {   // lane l reads lane l - N
    return __builtin_amdgcn_update_dpp(0, v, 0x110 + N, 0xf, 0xf, true);
}
template <int N>
__device__ __forceinline__ int dpp_shl(int v) {   // lane l reads lane l + N
    return __builtin_amdgcn_update_dpp(0, v, 0x100 + N, 0xf, 0xf, true);
}

// one step of the segmented inclusive scan: lanes that start a segment keep their value
template <int N>
__device__ __forceinline__ void scan_step(Run32 &v, int &flag) {
    const bool keep = flag != 0;
    const uint32_t qx = v.qx + (uint32_t)dpp_shr<N>((int)v.qx), qy = v.qy + (uint32_t)dpp_shr<N>((int)v.qy), qz = v.qz + (uint32_t)dpp_shr<N>((int)v.qz);
    const uint32_t cr = v.cr + (uint32_t)dpp_shr<N>((int)v.cr), gb = v.gb + (uint32_t)dpp_shr<N>((int)v.gb);
    const uint32_t tile = v.tile | (uint32_t)dpp_shr<N>((int)v.tile);
    v.qx = keep ? v.qx : qx; v.qy = keep ? v.qy : qy; v.qz = keep ? v.qz : qz;
    v.cr = keep ? v.cr : cr; v.gb = keep ? v.gb : gb; v.tile = keep ? v.tile : tile;
    flag |= dpp_shr<N>(flag);
}

// Two consecutive leaf faces of one axis, wave-uniform: faces mc and mc + 1 with their thresholds.
struct FaceCache {
    int mc;
    float tlo, thi;
    int cb;   // voxel index (of floor(p * inv_leaf)) that is cell 0 of leaf mc - 1:  ib + 64 * (mc - 1) - 2
};

struct PointOut {
    uint32_t key;   // cell inside the leaf grid, KEY_EMPTY if the point is skipped
    uint32_t nn;    // MODE 1: leaf relative to the cached faces, n0 | n1 << 2 | n2 << 4 with leaf_a = mc_a - 1 + n_a
    // One set of registers for two things that are never alive together: leaf lattice coordinates (MODE 0 / 2,
    // and MODE 1 once a step has gone the slow way), or the voxel index relative to cb (MODE 1, window test).
    union { int l0; int u0; };
    union { int l1; int u1; };
    union { int l2; int u2; };
    uint32_t q0, q1, q2; // biased fixed-point offsets inside the voxel (>= 0)
    bool seen;      // the point exists and is finite
};

// One coordinate: cell c inside the leaf grid, leaf (n or l), offset q inside the voxel.
// MODE 0: plain grid (bricks on the voxel lattice); 1: octree leaves by face thresholds; 2: octree leaves by f64 division.
template <int MODE>
__device__ __forceinline__ void axis_cell(const K1Params &P, int ib, const FaceCache &fc, int axis, float f, int &u, int &n, int &l, int &c,
                                          uint32_t &q) {
    const float prod = __fmul_rn(f, P.inv_leaf);
    const float g = floorf(prod);                        // pcl::VoxelGrid: floor(p * inverse_leaf_size), fp32 product
    const int ti = (int)g;                               // v_cvt_i32_f32 (saturating; non-finite points are masked by the caller)
    if (MODE == 1) {
        // leaf = (face mc - 1) + [f >= T(mc)] + [f >= T(mc + 1)], valid while the voxel lies between faces mc - 1/2 and mc + 3/2
        u = ti - fc.cb;
        n = (f >= fc.tlo ? -1 : 0) + (f >= fc.thi ? -1 : 0);   // minus the count: c is then one shift-and-add
        c = (n << 6) + u;
    } else {
        const int t = ti - ib;
        if (MODE == 0) l = t >> 6;
        else l = (int)floor(((double)f - P.mn0[axis]) / P.res);   // genOctreeKeyforPoint
        c = t - 64 * l + 2;
    }
    q = voxel_offset(prod);
}

template <int MODE>
__device__ __forceinline__ PointOut point_key(const K1Params &P, const FaceCache &f0, const FaceCache &f1, const FaceCache &f2, float fx, float fy,
                                              float fz, bool present) {
    PointOut o;
    int c0, c1, c2, n0 = 0, n1 = 0, n2 = 0;
    axis_cell<MODE>(P, P.ib0, f0, 0, fx, o.u0, n0, o.l0, c0, o.q0);
    axis_cell<MODE>(P, P.ib1, f1, 1, fy, o.u1, n1, o.l1, c1, o.q1);
    axis_cell<MODE>(P, P.ib2, f2, 2, fz, o.u2, n2, o.l2, c2, o.q2);
    o.nn = MODE == 1 ? (uint32_t)(-(n0 + (n1 << 2) + (n2 << 4))) : 0u;   // MODE 1: n_a = -(leaf position) here
    // Non-finite points are skipped as the octree does (addPointsFromInputCloud: isFinite).  One test for
    // the three coordinates: the sum is NaN or Inf iff one of them is (or they are beyond any sane range).
    o.seen = present && __builtin_isfinite(fx + fy + fz);
    // memory safety: a cell outside the leaf grid must never become a record address
    const uint32_t cm = max(max((uint32_t)c0, (uint32_t)c1), (uint32_t)c2);
    o.key = (o.seen && cm < (uint32_t)GRID_DIM) ? (uint32_t)__umul24(__umul24((uint32_t)c2, GRID_DIM) + (uint32_t)c1, GRID_DIM) + (uint32_t)c0 : KEY_EMPTY;
    return o;
}

// The same for a step whose voxels do not fit between one pair of cached faces per axis (a scan line
// wrapping around, a sparse cloud): every point looks up the two faces next to its own voxel in the
// threshold table in LDS.  Same arithmetic, same results, six LDS reads per point more.
__device__ __forceinline__ PointOut point_key_lookup(const K1Params &P, const float *faces, float fx, float fy, float fz, bool present, bool &off_table) {
    PointOut o;
    o.nn = 0;
    int c[3], l[3];
    uint32_t q[3];
    const float f[3] = {fx, fy, fz};
    const int ib[3] = {P.ib0, P.ib1, P.ib2}, fb[3] = {P.fb0, P.fb1, P.fb2};
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float prod = __fmul_rn(f[a], P.inv_leaf);
        const float g = floorf(prod);
        const int t = (int)g - ib[a];
        const int m = (t + 32) >> 6;                         // the face nearest to this voxel
        const unsigned i = (unsigned)(m - fb[a]);
        const bool in_table = i + 1u < (unsigned)FACES;
        ok &= in_table;
        const unsigned ii = in_table ? i : 0u;
        const float tlo = faces[a * FACES + ii], thi = faces[a * FACES + ii + 1];
        l[a] = m - 1 + (f[a] >= tlo ? 1 : 0) + (f[a] >= thi ? 1 : 0);
        c[a] = t - 64 * l[a] + 2;
        q[a] = voxel_offset(prod);
    }
    o.l0 = l[0]; o.l1 = l[1]; o.l2 = l[2];
    o.q0 = q[0]; o.q1 = q[1]; o.q2 = q[2];
    o.seen = present && __builtin_isfinite(fx + fy + fz);
    off_table |= o.seen && !ok;
    const uint32_t cm = max(max((uint32_t)c[0], (uint32_t)c[1]), (uint32_t)c[2]);
    o.key = (o.seen && ok && cm < (uint32_t)GRID_DIM) ? (uint32_t)__umul24(__umul24((uint32_t)c[2], GRID_DIM) + (uint32_t)c[1], GRID_DIM) + (uint32_t)c[0] : KEY_EMPTY;
    return o;
}

// r,g,b,tile bytes of one point as addends of the run sums: byte permutes instead of shifts and masks
struct PointAdd {
    uint32_t cr;     // count << 16 | r
    uint32_t gb;     // g << 16 | b
    uint32_t tile;
};
__device__ __forceinline__ PointAdd point_add(uint32_t w) {
    PointAdd a;
    a.cr = (w & 0xffu) | 0x10000u;
    a.gb = __builtin_amdgcn_perm(0u, w, 0x0c010c02u);   // bytes [b, 0, g, 0]
    a.tile = w >> 24;
    return a;
}
__device__ __forceinline__ void add_point(Run32 &r, const PointOut &o, const PointAdd &a) {
    r.qx += o.q0; r.qy += o.q1; r.qz += o.q2;
    r.cr += a.cr; r.gb += a.gb; r.tile |= a.tile;
}

// v_min3_f32 / v_max3_f32 on operands known to be numbers
__device__ __forceinline__ float min3f(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float max3f(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

template <int MODE>
__global__ void __launch_bounds__(K1_THREADS) voxel_accumulate_kernel(K1Params P, const float *__restrict__ x, const float *__restrict__ y,
                                                                     const float *__restrict__ z, const uint32_t *__restrict__ rgbt, VoxWork W) {
    extern __shared__ __align__(16) unsigned char k1_smem[];
    LdsTable &L = *reinterpret_cast<LdsTable *>(k1_smem);
    // stage switches for timing experiments exist in -DCWIPC_DEBUG_KNOBS builds only (results are wrong when set)
#ifdef CWIPC_DEBUG_KNOBS
    const uint32_t ablate = P.ablate;
#else
    constexpr uint32_t ablate = 0u;
#endif

    const int lane = threadIdx.x & 63;
    // everything that is the same for the whole wave lives in SGPRs
    const uint32_t range = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * K1_WAVES + (threadIdx.x >> 6)));
    float bn0 = FLT_MAX, bn1 = FLT_MAX, bn2 = FLT_MAX, bx0 = -FLT_MAX, bx1 = -FLT_MAX, bx2 = -FLT_MAX;
    uint32_t err = 0;
    // this wave's range [lo, hi); planes are padded to a multiple of 256 points, so whole steps can be loaded
    const uint32_t lo = range * P.per_wave;
    const uint32_t hi = min(lo + P.per_wave, P.n);
    const int npts = lo < hi ? (int)(hi - lo) : 0;
    const float4 *vx = reinterpret_cast<const float4 *>(x + lo) + lane;
    const float4 *vy = reinterpret_cast<const float4 *>(y + lo) + lane;
    const float4 *vz = reinterpret_cast<const float4 *>(z + lo) + lane;
    const uint4 *vw = reinterpret_cast<const uint4 *>(rgbt + lo) + lane;
    // the first step's loads go out before the table is initialised: their latency hides behind it
    float4 cx = make_float4(0, 0, 0, 0), cy = cx, cz = cx;
    uint4 cw = make_uint4(0, 0, 0, 0);
    if (npts > 0) { cx = vx[0]; cy = vy[0]; cz = vz[0]; cw = vw[0]; }

    if (!(ablate & 128u))
    for (int i = threadIdx.x; i < LTAB; i += K1_THREADS) {
        L.key[i] = KEY_EMPTY; L.tile[i] = 0;
        L.a[i] = 0; L.b[i] = 0; L.c[i] = 0; L.d[i] = 0;
    }
    if (MODE == 1) {
        for (int i = threadIdx.x; i < 3 * FACES; i += K1_THREADS) L.faces[i] = W.faces[i];
    }
    if (threadIdx.x < HIST) { L.htag[threadIdx.x] = 0; L.hcnt[threadIdx.x] = 0; }
    if (threadIdx.x < LOCAL_LEAVES) { L.leaf_tab[threadIdx.x] = 0ull; L.leaf_gid[threadIdx.x] = 0xffffffffu; }
    L.nn_leaf[threadIdx.x >> 6][threadIdx.x & 63] = 0xffffffffu;
    if (threadIdx.x == 0) { L.nfresh = 0; L.nfallback = 0; L.nused = 0; }
    __syncthreads();

    // wave-uniform caches: two leaf faces per axis, the last leaf and its id
    FaceCache fc0, fc1, fc2;
    fc0.mc = fc1.mc = fc2.mc = -(1 << 24);   // covers nothing yet
    fc0.tlo = fc0.thi = fc1.tlo = fc1.thi = fc2.tlo = fc2.thi = 0.f;
    fc0.cb = fc1.cb = fc2.cb = 1 << 30;
    int cl0 = 0, cl1 = 0, cl2 = 0;
    uint32_t cache_id = 0xffffffffu;
    bool cache_valid = false;

#pragma unroll 1
    for (int off = 0; off < npts; off += WAVE_STEP) {
        // keep the next step's 64 bytes per lane in flight while this step is processed
        float4 nx = cx, ny = cy, nz = cz;
        uint4 nw = cw;
        if (off + WAVE_STEP < npts) {
            const int v = (off + WAVE_STEP) >> 2;
            nx = vx[v]; ny = vy[v]; nz = vz[v]; nw = vw[v];
        }
        const int left = npts - off - lane * 4;   // points of this lane that exist: min(left, 4)

        if (ablate & 1u) {   // diagnostics: loads only
            bn0 = fminf(bn0, cx.x + cx.y + cx.z + cx.w + cy.x + cy.y + cy.z + cy.w + cz.x + cz.y + cz.z + cz.w + __uint_as_float(cw.x ^ cw.y ^ cw.z ^ cw.w));
            cx = nx; cy = ny; cz = nz; cw = nw;
            continue;
        }

        // ---- per point: cell, leaf, fixed-point offsets (branch-free) ----
        PointOut o0 = point_key<MODE>(P, fc0, fc1, fc2, cx.x, cy.x, cz.x, left > 0);
        PointOut o1 = point_key<MODE>(P, fc0, fc1, fc2, cx.y, cy.y, cz.y, left > 1);
        PointOut o2 = point_key<MODE>(P, fc0, fc1, fc2, cx.z, cy.z, cz.z, left > 2);
        PointOut o3 = point_key<MODE>(P, fc0, fc1, fc2, cx.w, cy.w, cz.w, left > 3);

        // ---- box of the wave's range (input of the octree replay): skipped points stay out of it ----
        if (__ballot(!(o0.seen && o1.seen && o2.seen && o3.seen)) == 0ull) {
            // (all twelve coordinates are finite here; written as instructions because fminf / fmaxf make the
            // compiler quiet every operand first, which costs more than the minimum itself)
            bn0 = min3f(min3f(bn0, cx.x, cx.y), cx.z, cx.w); bx0 = max3f(max3f(bx0, cx.x, cx.y), cx.z, cx.w);
            bn1 = min3f(min3f(bn1, cy.x, cy.y), cy.z, cy.w); bx1 = max3f(max3f(bx1, cy.x, cy.y), cy.z, cy.w);
            bn2 = min3f(min3f(bn2, cz.x, cz.y), cz.z, cz.w); bx2 = max3f(max3f(bx2, cz.x, cz.y), cz.z, cz.w);
        } else {
            // a ragged last step or non-finite points: NaN is the neutral element of v_min / v_max
            const float nan = __uint_as_float(0x7fc00000u);
            auto box = [&](bool seen, float fx, float fy, float fz) {
                const float sx = seen ? fx : nan, sy = seen ? fy : nan, sz = seen ? fz : nan;
                bn0 = fminf(bn0, sx); bx0 = fmaxf(bx0, sx);
                bn1 = fminf(bn1, sy); bx1 = fmaxf(bx1, sy);
                bn2 = fminf(bn2, sz); bx2 = fmaxf(bx2, sz);
            };
            box(o0.seen, cx.x, cy.x, cz.x); box(o1.seen, cx.y, cy.y, cz.y); box(o2.seen, cx.z, cy.z, cz.z); box(o3.seen, cx.w, cy.w, cz.w);
        }

        bool slow_step = false;   // MODE 1: this step's points carry leaf coordinates instead of positions around the cached faces
        if (MODE == 1) {
            // Are all voxels of this step between the cached faces?  u - 34 = voxel - (64 mc - 32) must lie in [0, 128).
            // Cheap test on the lane's extremes first; points that do not count (absent, non-finite) can only
            // raise a false alarm, which the exact test below sorts out.
            auto spread = [](int a, int b, int c, int d) {
                const int lo = min(min(a, b), min(c, d)), hi = max(max(a, b), max(c, d));
                return (uint32_t)(lo - 34) | (uint32_t)(hi - 34);
            };
            const uint32_t out = spread(o0.u0, o1.u0, o2.u0, o3.u0) | spread(o0.u1, o1.u1, o2.u1, o3.u1) | spread(o0.u2, o1.u2, o2.u2, o3.u2);
            if (__builtin_expect(__ballot(out >= 128u) != 0ull, 0)) {
                auto outside = [](const PointOut &o) {
                    return o.seen && (((uint32_t)(o.u0 - 34) | (uint32_t)(o.u1 - 34) | (uint32_t)(o.u2 - 34)) >= 128u);
                };
                if (__ballot(outside(o0) || outside(o1) || outside(o2) || outside(o3)) != 0ull) {
                    // Where do the voxels of this step lie?  (t = u + cb - ib, lowest and highest per axis)
                    const int big = 1 << 30;
                    int w0 = big, w1 = big, w2 = big, v0 = -big, v1 = -big, v2 = -big;
                    auto span = [&](const PointOut &o) {
                        if (o.seen) {
                            w0 = min(w0, o.u0); w1 = min(w1, o.u1); w2 = min(w2, o.u2);
                            v0 = max(v0, o.u0); v1 = max(v1, o.u1); v2 = max(v2, o.u2);
                        }
                    };
                    span(o0); span(o1); span(o2); span(o3);
                    for (int sft = 32; sft > 0; sft >>= 1) {
                        w0 = min(w0, __shfl_xor(w0, sft, 64)); w1 = min(w1, __shfl_xor(w1, sft, 64)); w2 = min(w2, __shfl_xor(w2, sft, 64));
                        v0 = max(v0, __shfl_xor(v0, sft, 64)); v1 = max(v1, __shfl_xor(v1, sft, 64)); v2 = max(v2, __shfl_xor(v2, sft, 64));
                    }
                    // A pair of faces covers 128 voxels.  If the step fits into that on every axis, move the
                    // caches to the lowest face it needs (thresholds come from the table the host computed)
                    // and redo it; if not, its points look their faces up one by one.
                    bool fits = true, off_table = false;
                    auto plan = [&](const FaceCache &fc, int umin, int umax, int ib, int fb, int &m) {
                        m = fc.mc;
                        if (umin == big) return;   // no point on this step at all
                        const int tmin = umin + fc.cb - ib, tmax = umax + fc.cb - ib;
                        m = (tmin + 32) >> 6;      // nearest face of the lowest voxel
                        fits &= tmax - (64 * m - 32) < 128;
                        fits &= (unsigned)(m - fb) + 1u < (unsigned)FACES;
                    };
                    int m0, m1, m2;
                    plan(fc0, __builtin_amdgcn_readfirstlane(w0), __builtin_amdgcn_readfirstlane(v0), P.ib0, P.fb0, m0);
                    plan(fc1, __builtin_amdgcn_readfirstlane(w1), __builtin_amdgcn_readfirstlane(v1), P.ib1, P.fb1, m1);
                    plan(fc2, __builtin_amdgcn_readfirstlane(w2), __builtin_amdgcn_readfirstlane(v2), P.ib2, P.fb2, m2);
                    if (fits) {
                        auto refill = [&](FaceCache &fc, int m, int ib, int fb, int axis) {
                            if (m == fc.mc) return;
                            const unsigned i = (unsigned)(m - fb);
                            fc.mc = m;
                            fc.tlo = L.faces[axis * FACES + i];
                            fc.thi = L.faces[axis * FACES + i + 1];
                            fc.cb = ib + 64 * (m - 1) - 2;
                        };
                        refill(fc0, m0, P.ib0, P.fb0, 0);
                        refill(fc1, m1, P.ib1, P.fb1, 1);
                        refill(fc2, m2, P.ib2, P.fb2, 2);
                        L.nn_leaf[threadIdx.x >> 6][lane] = 0xffffffffu;   // relative leaf positions mean other leaves now
                        o0 = point_key<MODE>(P, fc0, fc1, fc2, cx.x, cy.x, cz.x, left > 0);
                        o1 = point_key<MODE>(P, fc0, fc1, fc2, cx.y, cy.y, cz.y, left > 1);
                        o2 = point_key<MODE>(P, fc0, fc1, fc2, cx.z, cy.z, cz.z, left > 2);
                        o3 = point_key<MODE>(P, fc0, fc1, fc2, cx.w, cy.w, cz.w, left > 3);
                    } else {
                        slow_step = true;
                        o0 = point_key_lookup(P, L.faces, cx.x, cy.x, cz.x, left > 0, off_table);
                        o1 = point_key_lookup(P, L.faces, cx.y, cy.y, cz.y, left > 1, off_table);
                        o2 = point_key_lookup(P, L.faces, cx.z, cy.z, cz.z, left > 2, off_table);
                        o3 = point_key_lookup(P, L.faces, cx.w, cy.w, cz.w, left > 3, off_table);
                        // beyond the table (more than 60 leaves from the first point): the host reruns the f64 variant
                        if (__ballot(off_table) != 0ull) err |= ERR_FACE_TABLE;
                    }
                }
            }
        }

        if (ablate & 2u) {   // diagnostics: loads + per-point arithmetic only
            bx0 = fmaxf(bx0, __uint_as_float((o0.key ^ o1.key ^ o2.key ^ o3.key) + (o0.q0 + o1.q1 + o2.q2 + o3.q0 + o0.nn + o1.nn + o2.nn + o3.nn) +
                                              (uint32_t)(o0.l0 + o1.l1 + o2.l2)));
            cx = nx; cy = ny; cz = nz; cw = nw;
            continue;
        }

        // ---- leaf ids ----
        if (MODE == 1 && !slow_step && !(ablate & 64u)) {
            // The leaf of a point is one of the 27 positions around the cached faces (nn); this wave's table
            // in LDS says which leaf that is.  A plain LDS read per point; the lookup behind it runs once
            // per position (and again after the face caches moved).
            uint32_t *tab = L.nn_leaf[threadIdx.x >> 6];
            uint32_t s0 = tab[o0.nn], s1 = tab[o1.nn], s2 = tab[o2.nn], s3 = tab[o3.nn];
            const auto unknown = [](const PointOut &o, uint32_t sl) { return o.key != KEY_EMPTY && sl == 0xffffffffu; };
            // (first a test that may raise a false alarm for points that do not count: one maximum instead of
            // four two-part conditions; the loop behind it looks closely)
            if (__builtin_expect(__ballot(max(max(s0, s1), max(s2, s3)) == 0xffffffffu) != 0ull, 0)) {
                for (;;) {
                    const uint32_t want = unknown(o0, s0) ? o0.nn : unknown(o1, s1) ? o1.nn : unknown(o2, s2) ? o2.nn : unknown(o3, s3) ? o3.nn : 0xffu;
                    const unsigned long long need = __ballot(want != 0xffu);
                    if (!need) break;
                    const int src = __ffsll((long long)need) - 1;
                    const uint32_t nnv = (uint32_t)__builtin_amdgcn_readlane((int)want, src);
                    const int q0 = fc0.mc - 1 + (int)(nnv & 3u), q1 = fc1.mc - 1 + (int)((nnv >> 2) & 3u), q2 = fc2.mc - 1 + (int)(nnv >> 4);
                    uint32_t found = 0;
                    if (lane == src) {
                        found = leaf_name(L, W, P, pack_leaf(q0, q1, q2));
                        if (found != 0xffffffffu) tab[nnv] = found;
                    }
                    found = (uint32_t)__builtin_amdgcn_readlane((int)found, src);
                    if (found == 0xffffffffu) {
                        // no room for this leaf: its points are dropped from this pass, the host runs another one
                        if (P.local_leaves) err |= ERR_LOCAL_LEAVES;
                        if (o0.nn == nnv) o0.key = KEY_EMPTY;
                        if (o1.nn == nnv) o1.key = KEY_EMPTY;
                        if (o2.nn == nnv) o2.key = KEY_EMPTY;
                        if (o3.nn == nnv) o3.key = KEY_EMPTY;
                    } else {
                        if (o0.nn == nnv) s0 = found;
                        if (o1.nn == nnv) s1 = found;
                        if (o2.nn == nnv) s2 = found;
                        if (o3.nn == nnv) s3 = found;
                    }
                }
            }
            // KEY_EMPTY stays all ones
            o0.key |= s0 << CELL_BITS; o1.key |= s1 << CELL_BITS; o2.key |= s2 << CELL_BITS; o3.key |= s3 << CELL_BITS;
        }
        if ((MODE != 1 || __builtin_expect(slow_step, 0)) && !(ablate & 64u)) {
            // the points carry leaf lattice coordinates here; one leaf and its name are cached in scalar registers
            int mm = 0;
            mm |= o0.key != KEY_EMPTY ? (o0.l0 ^ cl0) | (o0.l1 ^ cl1) | (o0.l2 ^ cl2) : 0;
            mm |= o1.key != KEY_EMPTY ? (o1.l0 ^ cl0) | (o1.l1 ^ cl1) | (o1.l2 ^ cl2) : 0;
            mm |= o2.key != KEY_EMPTY ? (o2.l0 ^ cl0) | (o2.l1 ^ cl1) | (o2.l2 ^ cl2) : 0;
            mm |= o3.key != KEY_EMPTY ? (o3.l0 ^ cl0) | (o3.l1 ^ cl1) | (o3.l2 ^ cl2) : 0;
            const bool mism = mm != 0;
            if (cache_valid && __ballot(mism) == 0ull) {
                // the whole step lies in the cached leaf (the common case); KEY_EMPTY stays all ones
                const uint32_t hi_bits = cache_id << CELL_BITS;
                o0.key |= hi_bits; o1.key |= hi_bits; o2.key |= hi_bits; o3.key |= hi_bits;
            } else {
                // general case: resolve the distinct leaves of this step one at a time
                unsigned pend = (o0.key != KEY_EMPTY ? 1u : 0u) | (o1.key != KEY_EMPTY ? 2u : 0u) | (o2.key != KEY_EMPTY ? 4u : 0u) |
                                (o3.key != KEY_EMPTY ? 8u : 0u);
                for (;;) {
                    const unsigned long long need = __ballot(pend != 0u);
                    if (!need) break;
                    const int src = __ffsll((long long)need) - 1;
                    const int slot = __ffs((int)pend) - 1;   // meaningful in lane src
                    const int m0 = slot == 0 ? o0.l0 : slot == 1 ? o1.l0 : slot == 2 ? o2.l0 : o3.l0;
                    const int m1 = slot == 0 ? o0.l1 : slot == 1 ? o1.l1 : slot == 2 ? o2.l1 : o3.l1;
                    const int m2 = slot == 0 ? o0.l2 : slot == 1 ? o1.l2 : slot == 2 ? o2.l2 : o3.l2;
                    const int s0 = __builtin_amdgcn_readlane(m0, src), s1 = __builtin_amdgcn_readlane(m1, src), s2 = __builtin_amdgcn_readlane(m2, src);
                    if (!(cache_valid && s0 == cl0 && s1 == cl1 && s2 == cl2)) {
                        uint32_t found = 0;
                        if (lane == src) found = leaf_name(L, W, P, pack_leaf(s0, s1, s2));
                        cache_id = (uint32_t)__builtin_amdgcn_readlane((int)found, src);
                        if (P.local_leaves && cache_id == 0xffffffffu) err |= ERR_LOCAL_LEAVES;
                        cl0 = s0; cl1 = s1; cl2 = s2;
                        cache_valid = true;
                    }
                    const uint32_t hi_bits = cache_id << CELL_BITS;
                    const bool lost = cache_id == 0xffffffffu;
                    if ((pend & 1u) && o0.l0 == s0 && o0.l1 == s1 && o0.l2 == s2) { pend &= ~1u; o0.key = lost ? KEY_EMPTY : (o0.key | hi_bits); }
                    if ((pend & 2u) && o1.l0 == s0 && o1.l1 == s1 && o1.l2 == s2) { pend &= ~2u; o1.key = lost ? KEY_EMPTY : (o1.key | hi_bits); }
                    if ((pend & 4u) && o2.l0 == s0 && o2.l1 == s1 && o2.l2 == s2) { pend &= ~4u; o2.key = lost ? KEY_EMPTY : (o2.key | hi_bits); }
                    if ((pend & 8u) && o3.l0 == s0 && o3.l1 == s1 && o3.l2 == s2) { pend &= ~8u; o3.key = lost ? KEY_EMPTY : (o3.key | hi_bits); }
                }
            }
        }

        // ---- runs inside the lane ----
        // A lane's 4 consecutive points form 1 run (the usual case) or a head run, a tail run and up to two
        // runs in between.  The tail (the whole lane if it is one run) takes part in a segmented scan over
        // lanes; the head is handed to the previous lane, whose chain it ends; a run in between is complete
        // as it is.  So a run that spans several lanes is inserted into the workgroup table once, by the lane
        // where its chain ends, and most steps need one table insert per lane at most (LDS atomics are the
        // scarcest resource of this kernel).
        const uint32_t k0 = o0.key, k1 = o1.key, k2 = o2.key, k3 = o3.key;
        const bool e1 = k1 == k0, e2 = k2 == k1, e3 = k3 == k2;
        const int nb = (e1 ? 0 : 1) + (e2 ? 0 : 1) + (e3 ? 0 : 1);   // boundaries inside the lane
        const bool single = nb == 0, multi = nb != 0;
        const PointAdd a0 = point_add(cw.x), a1 = point_add(cw.y), a2 = point_add(cw.z), a3 = point_add(cw.w);
        Run32 all;   // the four points together
        all.key = k3;
        all.qx = (o0.q0 + o1.q0) + (o2.q0 + o3.q0);
        all.qy = (o0.q1 + o1.q1) + (o2.q1 + o3.q1);
        all.qz = (o0.q2 + o1.q2) + (o2.q2 + o3.q2);
        all.cr = (a0.cr + a1.cr) + (a2.cr + a3.cr);
        all.gb = (a0.gb + a1.gb) + (a2.gb + a3.gb);
        all.tile = (a0.tile | a1.tile) | (a2.tile | a3.tile);
        Run32 H;     // head: the points before the first boundary
        {
            const uint32_t m1 = e1 ? ~0u : 0u, m2 = (e1 && e2) ? ~0u : 0u;
            H.key = k0;
            H.qx = o0.q0 + (o1.q0 & m1) + (o2.q0 & m2);
            H.qy = o0.q1 + (o1.q1 & m1) + (o2.q1 & m2);
            H.qz = o0.q2 + (o1.q2 & m1) + (o2.q2 & m2);
            H.cr = a0.cr + (a1.cr & m1) + (a2.cr & m2);
            H.gb = a0.gb + (a1.gb & m1) + (a2.gb & m2);
            H.tile = a0.tile | (a1.tile & m1) | (a2.tile & m2);
        }
        Run32 T;     // tail: the points after the last boundary
        {
            const uint32_t n2 = e3 ? ~0u : 0u, n1 = (e3 && e2) ? ~0u : 0u;
            T.key = k3;
            T.qx = o3.q0 + (o2.q0 & n2) + (o1.q0 & n1);
            T.qy = o3.q1 + (o2.q1 & n2) + (o1.q1 & n1);
            T.qz = o3.q2 + (o2.q2 & n2) + (o1.q2 & n1);
            T.cr = a3.cr + (a2.cr & n2) + (a1.cr & n1);
            T.gb = a3.gb + (a2.gb & n2) + (a1.gb & n1);
            T.tile = a3.tile | (a2.tile & n2) | (a1.tile & n1);
        }
        Run32 X;     // what the lane contributes to the scan
        X.key = k3;
        X.qx = single ? all.qx : T.qx; X.qy = single ? all.qy : T.qy; X.qz = single ? all.qz : T.qz;
        X.cr = single ? all.cr : T.cr; X.gb = single ? all.gb : T.gb; X.tile = single ? all.tile : T.tile;
        // ---- segmented inclusive scan over chains of lanes; chains are cut every 8 lanes so that three
        // DPP steps (1, 2, 4) cover them completely
        const uint32_t prev_xkey = (uint32_t)dpp_shr<1>((int)k3);   // 0 in the first lane of a row of 16
        const int flag0 = (single && (lane & 7) != 0 && prev_xkey == k0) ? 0 : 1;   // 1: the lane starts a chain
        int flag = flag0;
        if (!(ablate & 16u)) {
            scan_step<1>(X, flag);
            scan_step<2>(X, flag);
            scan_step<4>(X, flag);
        }
        // ---- where chains end; the head of the next lane, if it continues this chain ----
        // (cross-lane reads first, into plain variables: inside a short-circuit they would run with part
        // of the wave switched off and read zeros from those lanes)
        const bool row_first = (lane & 15) == 0, row_last = (lane & 15) == 15;
        const int next_flag0 = dpp_shl<1>(flag0), next_multi = dpp_shl<1>(multi ? 1 : 0);
        const uint32_t next_k0 = (uint32_t)dpp_shl<1>((int)k0);
        const bool tail_final = row_last | (next_flag0 != 0);
        const bool take = !row_last & (next_multi != 0) & (next_k0 == k3);
        if (!(ablate & 32u)) {
            const int tm = take ? -1 : 0;
            X.qx += (uint32_t)(dpp_shl<1>((int)H.qx) & tm);
            X.qy += (uint32_t)(dpp_shl<1>((int)H.qy) & tm);
            X.qz += (uint32_t)(dpp_shl<1>((int)H.qz) & tm);
            X.cr += (uint32_t)(dpp_shl<1>((int)H.cr) & tm);
            X.gb += (uint32_t)(dpp_shl<1>((int)H.gb) & tm);
            X.tile |= (uint32_t)(dpp_shl<1>((int)H.tile) & tm);
        }
        // this lane's head is taken by the previous lane under exactly the condition `take` has there
        const bool head_taken = multi & !row_first & (prev_xkey == k0);

        // ---- table inserts ----
        // what a lane has to insert, in this order: its chain (if it ends here), its head (if nobody took
        // it), the run(s) between head and tail.  Round 0 takes the first of them, which is all there is in
        // most steps of a scan-ordered cloud.
        if (!(ablate & 4u)) {
            const bool have_t = tail_final & (k3 != KEY_EMPTY);
            const bool have_h = multi & !head_taken & (k0 != KEY_EMPTY);
            Run32 M1, M2;   // nb == 2: one run in between (everything but head and tail); nb == 3: points 1 and 2
            M1.key = M2.key = KEY_EMPTY;
            M1.qx = M1.qy = M1.qz = M1.cr = M1.gb = M1.tile = 0;
            M2 = M1;
            if (__ballot(nb >= 2) != 0ull) {
                const bool three = nb == 3;
                const uint32_t sm = three ? ~0u : 0u;   // nb == 3: point 2 is a run of its own
                M1.key = nb >= 2 ? (e1 ? k2 : k1) : KEY_EMPTY;
                M1.qx = all.qx - H.qx - T.qx - (o2.q0 & sm);
                M1.qy = all.qy - H.qy - T.qy - (o2.q1 & sm);
                M1.qz = all.qz - H.qz - T.qz - (o2.q2 & sm);
                M1.cr = all.cr - H.cr - T.cr - (a2.cr & sm);
                M1.gb = all.gb - H.gb - T.gb - (a2.gb & sm);
                M1.tile = three ? a1.tile : (e1 ? a2.tile : (a1.tile | (e2 ? a2.tile : 0u)));
                M2.key = three ? k2 : KEY_EMPTY;
                M2.qx = o2.q0; M2.qy = o2.q1; M2.qz = o2.q2; M2.cr = a2.cr; M2.gb = a2.gb; M2.tile = a2.tile;
            }
            const bool have_m1 = M1.key != KEY_EMPTY, have_m2 = M2.key != KEY_EMPTY;
            const int i_h = have_t ? 1 : 0, i_m1 = i_h + (have_h ? 1 : 0), i_m2 = i_m1 + (have_m1 ? 1 : 0);
            const int n_items = i_m2 + (have_m2 ? 1 : 0);
#pragma unroll 1
            for (int round = 0; round < 4; round++) {
                if (round > 0 && __ballot(n_items > round) == 0ull) break;
                const bool s_t = have_t & (round == 0), s_h = have_h & (round == i_h), s_m1 = have_m1 & (round == i_m1), s_m2 = have_m2 & (round == i_m2);
                Run32 r;
                r.key = s_t ? k3 : s_h ? k0 : s_m1 ? M1.key : s_m2 ? M2.key : KEY_EMPTY;
                r.qx = s_t ? X.qx : s_h ? H.qx : s_m1 ? M1.qx : M2.qx;
                r.qy = s_t ? X.qy : s_h ? H.qy : s_m1 ? M1.qy : M2.qy;
                r.qz = s_t ? X.qz : s_h ? H.qz : s_m1 ? M1.qz : M2.qz;
                r.cr = s_t ? X.cr : s_h ? H.cr : s_m1 ? M1.cr : M2.cr;
                r.gb = s_t ? X.gb : s_h ? H.gb : s_m1 ? M1.gb : M2.gb;
                r.tile = s_t ? X.tile : s_h ? H.tile : s_m1 ? M1.tile : M2.tile;
                lds_insert(L, W, P, r, r.key != KEY_EMPTY);
            }
        }
        cx = nx; cy = ny; cz = nz; cw = nw;
    }

    if (ablate & 128u) { if (bn0 == 1.2345f) W.bboxes[0] = bn0 + bx0; return; }   // diagnostics: no epilogue at all
    // ---- errors of this wave, bounding box of its range (input of the octree replay) ----
    {
        for (int s = 32; s > 0; s >>= 1) err |= (uint32_t)__shfl_xor((int)err, s, 64);
        if (lane == 0 && err) atomicOr(&W.ctrl[C_ERR], err);
        const float lo3[3] = {bn0, bn1, bn2}, hi3[3] = {bx0, bx1, bx2};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            float vlo = lo3[a], vhi = hi3[a];
            for (int s = 32; s > 0; s >>= 1) {
                vlo = fminf(vlo, __shfl_down(vlo, s, 64));
                vhi = fmaxf(vhi, __shfl_down(vhi, s, 64));
            }
            if (lane == 0) {
                W.bboxes[(size_t)range * 6 + a] = vlo;
                W.bboxes[(size_t)range * 6 + 3 + a] = vhi;
            }
        }
    }

    // ---- flush: 8 lanes per table entry update one 64-byte record with returning adds ----
    // All adds of a lane are issued before the first result is looked at, so that their round
    // trips overlap (this is the serial tail of the kernel: nothing else is in flight any more).
    __syncthreads();
    if (P.local_leaves) {
        // local leaf slots -> global leaf ids (grids), one lookup per leaf and workgroup
        if (threadIdx.x < LOCAL_LEAVES) {
            // normally all there already (leaf_name); only a lookup that failed is tried again
            const unsigned long long lk = L.leaf_tab[threadIdx.x];
            if (lk != 0ull && L.leaf_gid[threadIdx.x] >= 0xfffffffeu) L.leaf_gid[threadIdx.x] = leaf_lookup(W, P.leaf_mask, lk);
        }
        __syncthreads();
    }
    const int sub = threadIdx.x & 7;
    constexpr int FLUSH_ITERS = LTAB / (K1_THREADS / 8);
    uint32_t fkey[FLUSH_ITERS];
    unsigned long long fold[FLUSH_ITERS];
    uint32_t used = 0;   // entries in use (lanes with sub == 0 count them)
#pragma unroll
    for (int it = 0; it < FLUSH_ITERS; it++) {
        const int e = (threadIdx.x >> 3) + it * (K1_THREADS / 8);
        uint32_t k = L.key[e];
        if (ablate & 8u) k = KEY_EMPTY;
        if (P.local_leaves && k != KEY_EMPTY) {
            const uint32_t gid = L.leaf_gid[k >> CELL_BITS];
            k = gid == 0xffffffffu ? KEY_EMPTY : ((gid << CELL_BITS) | (k & ((1u << CELL_BITS) - 1)));
        }
        fkey[it] = k;
        fold[it] = ~0ull;
        if (k == KEY_EMPTY) continue;
        used += sub == 0 ? 1u : 0u;
        const uint32_t t = L.tile[e];
        const unsigned long long ea = L.a[e], eb = L.b[e], ec = L.c[e], ed = L.d[e];
        const unsigned long long cnt = ed & 0xffffull;
        unsigned long long val;
        switch (sub) {
        case 0: val = ea; break;                                             // sum qx
        case 1: val = eb; break;
        case 2: val = ec & ((1ull << 40) - 1); break;
        case 3: val = (cnt << 32) | ((ed >> 16) & 0xffffffull); break;      // count << 32 | sum r
        case 4: val = ((ed >> 40) << 32) | (ec >> 40); break;               // sum g << 32 | sum b
        case 5:   // tile bits 0-3 as 16-bit contribution counters
            val = (unsigned long long)(t & 1u) | ((unsigned long long)((t >> 1) & 1u) << 16) | ((unsigned long long)((t >> 2) & 1u) << 32) |
                  ((unsigned long long)((t >> 3) & 1u) << 48);
            break;
        case 6:   // tile bits 4-7
            val = (unsigned long long)((t >> 4) & 1u) | ((unsigned long long)((t >> 5) & 1u) << 16) | ((unsigned long long)((t >> 6) & 1u) << 32) |
                  ((unsigned long long)((t >> 7) & 1u) << 48);
            break;
        default: val = 0; break;
        }
        fold[it] = atomicAdd(&record_ptr(W, k)[sub], val);
    }
#pragma unroll
    for (int it = 0; it < FLUSH_ITERS; it++) {
        const uint32_t k = fkey[it];
        if (sub == 3 && k != KEY_EMPTY && (fold[it] >> 32) == 0) {
            // first touch of this record in this call: list it, set its bit, count it in its bitmap slice
            const uint32_t at = atomicAdd(&L.nfresh, 1u);
            if (P.want_list) L.fresh[at] = k;
            mark_occupied(W, k);
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
    for (int off = 32; off > 0; off >>= 1) used += (uint32_t)__shfl_xor((int)used, off, 64);
    if ((threadIdx.x & 63) == 0 && used) atomicAdd(&L.nused, used);
    __syncthreads();
    if (threadIdx.x < HIST && L.htag[threadIdx.x]) atomicAdd(&W.seg_count[L.htag[threadIdx.x] - 1u], L.hcnt[threadIdx.x]);
    const uint32_t nfresh = L.nfresh;
    if (threadIdx.x == 0) {
        // how the table fared: the host sizes the workgroups of the next call by it
        if (L.nfallback) atomicAdd(&W.ctrl[C_FALLBACK], L.nfallback);
        atomicMax(&W.ctrl[C_MAXLOAD], L.nused);
        if (L.nused) atomicAdd(&W.ctrl[C_FLUSHED], L.nused);
    }
    if (!P.want_list) {
        // octree path: the finalize pass finds the records through the occupancy bitmaps, so the count is
        // all that is needed here, and nobody waits for this add
        if (threadIdx.x == 0 && nfresh) atomicAdd(&W.ctrl[C_COUNT], nfresh);
        return;
    }
    if (threadIdx.x == 0 && nfresh) L.fresh_base = atomicAdd(&W.ctrl[C_COUNT], nfresh);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nfresh; i += K1_THREADS) {
        const uint32_t idx = L.fresh_base + i;
        if (idx < P.list_cap) W.occupied[idx] = L.fresh[i];
        else atomicOr(&W.ctrl[C_ERR], ERR_LIST_FULL);
    }
}
