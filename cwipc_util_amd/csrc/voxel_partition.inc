// voxel_partition.inc -- the partition pass in front of the accumulate kernel for clouds whose points come in no spatial
// order (a fused multi-camera capture, a shuffled cloud).  Included by kernels_voxel.hip.
//
// Why: the accumulate kernel merges the points of a voxel in its workgroup's LDS table and touches the global records once per
// voxel and workgroup.  A workgroup's range of an unordered cloud holds ~as many voxels as points: the table overflows and
// every point becomes one cache-line atomic in HBM (10 M points: 1.0 ms instead of 0.06).  Moving the points into coarse spatial
// buckets first costs one extra read and write of the cloud (320 MB) and gives every workgroup of the accumulate kernel a range
// that lies in a few buckets, i.e. a few hundred voxels.  The octree's shape depends on the ORDER in which the points widen its
// bounding box, so the per-range boxes the replay kernel works on are those of the cloud as it came, computed by the counting
// kernel here; the accumulate kernel's own boxes (of the moved points) are thrown away.  Sums are integers: the order in which a
// voxel's points are added does not matter, and within a bucket it is whatever the LDS atomics make it.
//
//   partition_count     one workgroup per range (the ranges the accumulate kernel would use): bounding box of the range, bucket
//                       histogram of the range (LDS), left as a ROW of a table in global memory, and how many wave steps were
//                       scattered over many buckets (so that the host can tell when the partition is no longer needed)
//   partition_segsum    the rows added up sixteen at a time (one thread per bucket and segment)
//   partition_starts    one workgroup: per bucket the segments' sums turned into a running total over the segments, and the
//                       exclusive prefix of the buckets' totals = where each bucket starts
//   partition_scatter   one workgroup per range again: where its points of bucket b go is known before it starts (start of the
//                       bucket + the segments before its own + the rows of its segment before its own: sixteen loads per
//                       bucket), so nothing is reserved while it runs -- 4096 points at a time: rank inside the bucket by LDS
//                       atomics, points staged in LDS in bucket order and written out in runs
//
// Round 4.  Rounds 2 and 3 kept ONE counter per bucket in global memory: the counting kernel's workgroups added their histograms to
// it (248 workgroups x ~1500 occupied buckets: 248 atomics per address, all at the end of the kernel -- ~40 of its 64 us, found by
// running it with 2 x and 4 x the workgroups: 104, 162 us), and the scatter kernel, one workgroup per 4096 points, reserved its runs
// with one atomic per occupied bucket and chunk (2441 x ~2000 = 5 M atomics on 1500 addresses).  No atomic in global memory now.
//
// Bucket of a point: its voxel (the fp32 product and floor of pcl::VoxelGrid, as everywhere) >> 4 per axis, taken modulo 16:
// cells of 16^3 voxels, a quarter of an octree leaf per axis; clouds up to 256 voxels across map one cell to one bucket, larger
// ones fold over (two far-apart cells in one bucket: more voxels per bucket, nothing else).

constexpr int PART_BUCKETS = 4096;
constexpr int PART_CHUNK = 4096;     // points per workgroup of the scatter kernel (4 per lane)
constexpr int PART_SEG_ROWS = 16;    // rows (workgroups) per segment of the histogram table

__device__ __forceinline__ uint32_t part_bucket(float fx, float fy, float fz, float inv) {
    // (non-finite coordinates convert to something: such points do not count anywhere, they only have to be moved somewhere)
    const int cx = (int)floorf(__fmul_rn(fx, inv)) >> 4, cy = (int)floorf(__fmul_rn(fy, inv)) >> 4, cz = (int)floorf(__fmul_rn(fz, inv)) >> 4;
    return (uint32_t)((cx & 15) | ((cy & 15) << 4) | ((cz & 15) << 8));
}

// (per_wg: points of a workgroup's contiguous range; its waves take the range's 256-point steps one by one from a counter in
// LDS, as in the fast accumulate kernel -- fixed shares leave the last waves of a SIMD running alone -- and the range's box
// is one per workgroup)
__global__ void __launch_bounds__(K1_THREADS) partition_count_kernel(uint32_t n, uint32_t per_wg, float inv, const float *__restrict__ x,
                                                                    const float *__restrict__ y, const float *__restrict__ z, float *__restrict__ bboxes,
                                                                    uint32_t *__restrict__ rows, uint32_t *__restrict__ ctrl) {
    __shared__ uint32_t lh[PART_BUCKETS];
    __shared__ uint32_t next_step, scattered_steps;
    __shared__ float wbox[K1_WAVES][6];
    for (int i = threadIdx.x; i < PART_BUCKETS; i += K1_THREADS) lh[i] = 0;
    if (threadIdx.x == 0) { next_step = K1_WAVES; scattered_steps = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t chunk_lo = blockIdx.x * per_wg;
    const uint32_t chunk_hi = min(chunk_lo + per_wg, n);
    const int chunk_pts = chunk_lo < chunk_hi ? (int)(chunk_hi - chunk_lo) : 0;
    const int nsteps = (chunk_pts + WAVE_STEP - 1) / WAVE_STEP;
    auto load_step = [&](int step, float4 &ax, float4 &ay, float4 &az) __attribute__((always_inline)) {
        const size_t at = (size_t)chunk_lo + (size_t)(uint32_t)__builtin_amdgcn_readfirstlane(step) * WAVE_STEP;
        ax = reinterpret_cast<const float4 *>(x + at)[lane];
        ay = reinterpret_cast<const float4 *>(y + at)[lane];
        az = reinterpret_cast<const float4 *>(z + at)[lane];
    };
    auto grab = [&]() -> int {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&next_step, 1u);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        return t < (uint32_t)nsteps ? (int)t : -1;
    };
    float bn0 = FLT_MAX, bn1 = FLT_MAX, bn2 = FLT_MAX, bx0 = -FLT_MAX, bx1 = -FLT_MAX, bx2 = -FLT_MAX;
    const float nan = __uint_as_float(0x7fc00000u);
    uint32_t scattered = 0;
    float4 cx = make_float4(0, 0, 0, 0), cy = cx, cz = cx;
    int cur = wave < nsteps ? wave : -1;
    if (cur >= 0) load_step(cur, cx, cy, cz);
    int nxt = cur >= 0 ? grab() : -1;
#pragma unroll 1
    while (cur >= 0) {
        cur = __builtin_amdgcn_readfirstlane(cur);
        nxt = __builtin_amdgcn_readfirstlane(nxt);
        float4 nx = cx, ny = cy, nz = cz;   // the next step's loads are in flight while this one is counted
        if (nxt >= 0) load_step(nxt, nx, ny, nz);
        const int left = chunk_pts - cur * WAVE_STEP - lane * 4;
        uint32_t b_first = 0;
        auto one = [&](int i, float fx, float fy, float fz) {
            const bool present = left > i;
            // the box of the range exactly as the accumulate kernels build it: points that do not count stay out (NaN is the
            // neutral element of v_min / v_max)
            const bool seen = present && __builtin_isfinite(fx + fy + fz);
            const float sx = seen ? fx : nan, sy = seen ? fy : nan, sz = seen ? fz : nan;
            bn0 = fminf(bn0, sx); bx0 = fmaxf(bx0, sx);
            bn1 = fminf(bn1, sy); bx1 = fmaxf(bx1, sy);
            bn2 = fminf(bn2, sz); bx2 = fmaxf(bx2, sz);
            const uint32_t b = part_bucket(fx, fy, fz, inv);
            if (present) atomicAdd(&lh[b], 1u);
            if (i == 0) b_first = b;
        };
        one(0, cx.x, cy.x, cz.x); one(1, cx.y, cy.y, cz.y); one(2, cx.z, cy.z, cz.z); one(3, cx.w, cy.w, cz.w);
        // a step of a cloud in scan order lies in one or two buckets; count the steps where most lanes are somewhere else
        const uint32_t b_wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)b_first);
        if (__popcll(__ballot(left > 0 && b_first != b_wave)) > 32) scattered++;
        cx = nx; cy = ny; cz = nz;
        cur = nxt;
        if (cur >= 0) nxt = grab();
    }
    {
        const float lo3[3] = {bn0, bn1, bn2}, hi3[3] = {bx0, bx1, bx2};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            float vlo = lo3[a], vhi = hi3[a];
            for (int s = 32; s > 0; s >>= 1) {
                vlo = fminf(vlo, __shfl_down(vlo, s, 64));
                vhi = fmaxf(vhi, __shfl_down(vhi, s, 64));
            }
            if (lane == 0) { wbox[wave][a] = vlo; wbox[wave][3 + a] = vhi; }
        }
        // (one add per WORKGROUP to the control word below: one per wave -- 3968 atomics on one address at the end of the kernel --
        // was 25 of this kernel's 64 us, as every single counter in global memory is: ~6 ns per add, one after the other)
        if (lane == 0 && scattered) atomicAdd(&scattered_steps, scattered);
    }
    __syncthreads();
    if (threadIdx.x == 0 && scattered_steps) atomicAdd(&ctrl[C_SCATTER], scattered_steps);
    if (threadIdx.x < 6) {
        float v = wbox[0][threadIdx.x];
        for (int w = 1; w < K1_WAVES; w++) v = threadIdx.x < 3 ? fminf(v, wbox[w][threadIdx.x]) : fmaxf(v, wbox[w][threadIdx.x]);
        bboxes[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
    // this range's row of the table (every word of it: nothing clears the table between calls)
    reinterpret_cast<uint4 *>(rows + (size_t)blockIdx.x * PART_BUCKETS)[threadIdx.x] = reinterpret_cast<const uint4 *>(lh)[threadIdx.x];
    static_assert(PART_BUCKETS == 4 * K1_THREADS, "one uint4 of the row per thread");
}

// seg[s][b] = points of bucket b in the rows of segment s
__global__ void __launch_bounds__(256) partition_segsum_kernel(const uint32_t *__restrict__ rows, uint32_t nrows, uint32_t *__restrict__ seg) {
    const uint32_t s_ = blockIdx.x, b = blockIdx.y * 256 + threadIdx.x;
    const uint32_t w0 = s_ * PART_SEG_ROWS;
    uint32_t v[PART_SEG_ROWS];
#pragma unroll
    for (int k = 0; k < PART_SEG_ROWS; k++) v[k] = w0 + k < nrows ? rows[(size_t)(w0 + k) * PART_BUCKETS + b] : 0u;
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < PART_SEG_ROWS; k++) sum += v[k];
    seg[(size_t)s_ * PART_BUCKETS + b] = sum;
}

// block-wide exclusive scan of one value per thread (1024 threads); `wave_sums` is 16 words of LDS
__device__ __forceinline__ uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t *wave_sums, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, s, 64);
        if (lane >= s) inc += o;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < K1_WAVES; w++) {
        const uint32_t s = wave_sums[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    if (total) *total = all;
    return before + inc - v;
}

// seg[s][b] -> points of bucket b in the segments BEFORE s; start[b] = points in the buckets before b.  One workgroup, four
// buckets per thread (one uint4 of every segment's row).
__global__ void __launch_bounds__(K1_THREADS) partition_starts_kernel(uint32_t *__restrict__ seg, uint32_t nseg, uint32_t *__restrict__ start) {
    __shared__ uint32_t wave_sums[K1_WAVES];
    uint4 run = make_uint4(0, 0, 0, 0);
    for (uint32_t s0 = 0; s0 < nseg; s0 += 8) {
        uint4 c[8];
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = s0 + k < nseg ? reinterpret_cast<const uint4 *>(seg + (size_t)(s0 + k) * PART_BUCKETS)[threadIdx.x] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (s0 + k < nseg) reinterpret_cast<uint4 *>(seg + (size_t)(s0 + k) * PART_BUCKETS)[threadIdx.x] = run;
            run.x += c[k].x; run.y += c[k].y; run.z += c[k].z; run.w += c[k].w;
        }
    }
    const uint32_t at = block_exclusive_scan_1024(run.x + run.y + run.z + run.w, wave_sums, nullptr);
    reinterpret_cast<uint4 *>(start)[threadIdx.x] = make_uint4(at, at + run.x, at + run.x + run.y, at + run.x + run.y + run.z);
}

struct PartLds {
    uint32_t base[PART_BUCKETS];    // where this workgroup's next point of bucket b goes
    uint32_t cnt[PART_BUCKETS];     // points of the chunk per bucket
    float sx[PART_CHUNK], sy[PART_CHUNK], sz[PART_CHUNK];
    uint32_t sw[PART_CHUNK];
    uint16_t sb[PART_CHUNK];        // bucket of the point staged in this slot
    uint16_t lbase[PART_BUCKETS];   // first staging slot of the bucket
    uint32_t wave_sums[K1_WAVES];
};

// (per_wg: points of a workgroup's range -- the counting kernel's ranges, row blockIdx.x of the table is this workgroup's)
__global__ void __launch_bounds__(K1_THREADS) partition_scatter_kernel(uint32_t n, uint32_t per_wg, uint32_t padded, float inv, const float *__restrict__ x,
                                                                      const float *__restrict__ y, const float *__restrict__ z,
                                                                      const uint32_t *__restrict__ rgbt, float *__restrict__ ox, float *__restrict__ oy,
                                                                      float *__restrict__ oz, uint32_t *__restrict__ ow, const uint32_t *__restrict__ rows,
                                                                      const uint32_t *__restrict__ seg, const uint32_t *__restrict__ start) {
    extern __shared__ __align__(16) unsigned char part_smem[];
    PartLds &L = *reinterpret_cast<PartLds *>(part_smem);
    const uint32_t chunk_lo = blockIdx.x * per_wg;
    const uint32_t chunk_hi = min(chunk_lo + per_wg, n);
    auto load_chunk = [&](uint32_t at, float4 &ax, float4 &ay, float4 &az, uint4 &aw) __attribute__((always_inline)) {
        const uint32_t mine = at + threadIdx.x * 4u;
        ax = make_float4(0, 0, 0, 0); ay = ax; az = ax; aw = make_uint4(0, 0, 0, 0);
        if (mine < chunk_hi && mine < padded) {   // the planes are padded to whole wave steps: a float4 that starts below `padded` is all there
            ax = *reinterpret_cast<const float4 *>(x + mine); ay = *reinterpret_cast<const float4 *>(y + mine);
            az = *reinterpret_cast<const float4 *>(z + mine); aw = *reinterpret_cast<const uint4 *>(rgbt + mine);
        }
    };
    float4 cx, cy, cz;
    uint4 cw;
    load_chunk(chunk_lo, cx, cy, cz, cw);
    {
        // this workgroup's first slot of every bucket: the bucket's start, the segments before this row's, the rows of its segment before it
        const uint32_t s_ = blockIdx.x / PART_SEG_ROWS, w0 = s_ * PART_SEG_ROWS;
        uint4 at = reinterpret_cast<const uint4 *>(start)[threadIdx.x];
        const uint4 sg = reinterpret_cast<const uint4 *>(seg + (size_t)s_ * PART_BUCKETS)[threadIdx.x];
        uint4 r[PART_SEG_ROWS - 1];
#pragma unroll
        for (int k = 0; k < PART_SEG_ROWS - 1; k++)
            r[k] = w0 + k < blockIdx.x ? reinterpret_cast<const uint4 *>(rows + (size_t)(w0 + k) * PART_BUCKETS)[threadIdx.x] : make_uint4(0, 0, 0, 0);
        at.x += sg.x; at.y += sg.y; at.z += sg.z; at.w += sg.w;
#pragma unroll
        for (int k = 0; k < PART_SEG_ROWS - 1; k++) { at.x += r[k].x; at.y += r[k].y; at.z += r[k].z; at.w += r[k].w; }
        reinterpret_cast<uint4 *>(L.base)[threadIdx.x] = at;
        reinterpret_cast<uint4 *>(L.cnt)[threadIdx.x] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t at = chunk_lo; at < chunk_hi; at += PART_CHUNK) {
        // the next chunk's loads are in flight while this one is moved
        float4 nx, ny, nz;
        uint4 nw;
        load_chunk(at + PART_CHUNK, nx, ny, nz, nw);
        const uint32_t mine = at + threadIdx.x * 4u;
        const int left = mine < chunk_hi ? (int)min(chunk_hi - mine, 4u) : 0;
        const float fx[4] = {cx.x, cx.y, cx.z, cx.w}, fy[4] = {cy.x, cy.y, cy.z, cy.w}, fz[4] = {cz.x, cz.y, cz.z, cz.w};
        const uint32_t fw[4] = {cw.x, cw.y, cw.z, cw.w};
        uint32_t b[4], r[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            b[i] = part_bucket(fx[i], fy[i], fz[i], inv);
            r[i] = 0;
            if (i < left) r[i] = atomicAdd(&L.cnt[b[i]], 1u);   // rank among the chunk's points of this bucket
        }
        __syncthreads();
        uint4 c4;
        {
            c4 = reinterpret_cast<const uint4 *>(L.cnt)[threadIdx.x];   // four buckets per thread
            uint32_t first = block_exclusive_scan_1024(c4.x + c4.y + c4.z + c4.w, L.wave_sums, nullptr);
            const int bk = threadIdx.x * 4;
            L.lbase[bk] = (uint16_t)first; L.lbase[bk + 1] = (uint16_t)(first + c4.x); L.lbase[bk + 2] = (uint16_t)(first + c4.x + c4.y);
            L.lbase[bk + 3] = (uint16_t)(first + c4.x + c4.y + c4.z);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i < left) {
                const uint32_t slot = (uint32_t)L.lbase[b[i]] + r[i];
                L.sx[slot] = fx[i]; L.sy[slot] = fy[i]; L.sz[slot] = fz[i]; L.sw[slot] = fw[i];
                L.sb[slot] = (uint16_t)b[i];
            }
        }
        __syncthreads();
        const uint32_t have = min(chunk_hi - at, (uint32_t)PART_CHUNK);
        for (uint32_t j = threadIdx.x; j < have; j += K1_THREADS) {
            const uint32_t bk = L.sb[j];
            const uint32_t dst = L.base[bk] + (j - (uint32_t)L.lbase[bk]);   // consecutive slots of one bucket go to consecutive addresses
            ox[dst] = L.sx[j]; oy[dst] = L.sy[j]; oz[dst] = L.sz[j]; ow[dst] = L.sw[j];
        }
        __syncthreads();
        {
            // the buckets' next slots; the counts cleared for the next chunk
            uint4 bs = reinterpret_cast<const uint4 *>(L.base)[threadIdx.x];
            bs.x += c4.x; bs.y += c4.y; bs.z += c4.z; bs.w += c4.w;
            reinterpret_cast<uint4 *>(L.base)[threadIdx.x] = bs;
            reinterpret_cast<uint4 *>(L.cnt)[threadIdx.x] = make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        cx = nx; cy = ny; cz = nz; cw = nw;
    }
}
