// voxel_finalize.inc -- what runs behind the accumulate kernel of the voxel-grid downsample (included by kernels_voxel.hip): the
// octree replay that publishes the pass's control words, the finalize kernels of both variants (rank_emit: octree; grid_*: plain
// grid; sort keys + emit_and_clean: plain-grid index spaces beyond 2^28 cells), the clean-up kernel, and the first-point fetches.

// ---------------------------------------------------------------------------
// K2: octree bounding-box replay / global grid box
// ---------------------------------------------------------------------------
// Results straight into the host's pinned words: the host polls them instead of waiting for the stream
// (a blocking stream wait wakes up several microseconds late).
// Every control word travels as one 64-bit store with the sequence number in its upper half, so the host
// can tell word by word what has arrived: no release fence (a system-scope release writes back the whole
// L2, which K1 has just filled with dirty records) and no second store behind it.
__device__ __forceinline__ void publish(const uint32_t *ctrl, uint32_t *host_out, uint32_t seq) {
    const int tid = threadIdx.x;
    if (tid < C_SEQ) {
        const uint32_t v = __hip_atomic_load(&ctrl[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(host_out) + tid, ((unsigned long long)seq << 32) | v, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Growth of pcl::octree::OctreePointCloud's box is sequential in input order, but a range
// whose box lies inside the current octree box cannot trigger a growth step, so only the few
// ranges that do are re-read point by point.
__global__ void __launch_bounds__(1024) octree_replay_kernel(VoxParams P, const float *__restrict__ x, const float *__restrict__ y,
                                                            const float *__restrict__ z, const float *__restrict__ bboxes,
                                                            uint32_t *__restrict__ ctrl, const unsigned long long *__restrict__ leaf_keys,
                                                            uint32_t leaf_cap, uint32_t *__restrict__ next_head, uint32_t next_head_words,
                                                            uint32_t *__restrict__ host_out, uint32_t seq) {
    // housekeeping this single workgroup has threads to spare for: it zeroes the control block the NEXT call
    // on this workspace will use (the two blocks alternate, so no memset sits in front of that call's first
    // kernel) -- at the very end, after the results have gone out to the host, which is waiting for them
    const auto zero_next_head = [&]() {
        for (uint32_t i = threadIdx.x; i < next_head_words; i += 1024) next_head[i] = 0u;
    };
    __shared__ double s_mn[3], s_mx[3];
    __shared__ int s_resolved;
    __shared__ int s_depth;
    __shared__ long long s_shift[3];
    __shared__ unsigned long long s_first;
    __shared__ int s_events;
    const int tid = threadIdx.x;
    const uint32_t nranges = P.nranges;

    if (!P.leaf_split) {
        // plain pcl::VoxelGrid: getMinMax3D, the 2^31-cell check, min_b / div_b
        __shared__ float s_red[6][16];
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (uint32_t c = tid; c < nranges; c += 1024) {
            for (int a = 0; a < 3; a++) {
                lo[a] = fminf(lo[a], bboxes[(size_t)c * 6 + a]);
                hi[a] = fmaxf(hi[a], bboxes[(size_t)c * 6 + 3 + a]);
            }
        }
        for (int a = 0; a < 3; a++) {
            for (int off = 32; off > 0; off >>= 1) {
                lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64));
                hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64));
            }
            if ((tid & 63) == 0) { s_red[a][tid >> 6] = lo[a]; s_red[3 + a][tid >> 6] = hi[a]; }
        }
        __syncthreads();
        if (tid == 0) {
            float mn[3], mx[3];
            for (int a = 0; a < 3; a++) {
                mn[a] = s_red[a][0]; mx[a] = s_red[3 + a][0];
                for (int w = 1; w < 16; w++) { mn[a] = fminf(mn[a], s_red[a][w]); mx[a] = fmaxf(mx[a], s_red[3 + a][w]); }
            }
            long long d[3];
            int minb[3], divb[3];
            for (int a = 0; a < 3; a++) {
                d[a] = (long long)(__fmul_rn(__fsub_rn(mx[a], mn[a]), P.inv_leaf)) + 1;
                minb[a] = (int)floorf(__fmul_rn(mn[a], P.inv_leaf));
                int maxb = (int)floorf(__fmul_rn(mx[a], P.inv_leaf));
                divb[a] = maxb - minb[a] + 1;
            }
            if (d[0] * d[1] * d[2] > (long long)INT32_MAX) atomicOr(&ctrl[C_ERR], ERR_GRID_OVERFLOW);
            for (int a = 0; a < 3; a++) { ctrl[C_MINB + a] = (uint32_t)minb[a]; ctrl[C_DIVB + a] = (uint32_t)divb[a]; }
        }
        __syncthreads();
        // results straight into the host's pinned words: the host only waits for the stream
        publish(ctrl, host_out, seq);
        zero_next_head();
        return;
    }

    if (tid == 0) {
        for (int a = 0; a < 3; a++) { s_mn[a] = P.mn0[a]; s_mx[a] = P.mx0[a]; s_shift[a] = 0; }
        s_depth = P.depth0;
        s_events = 0;
    }
    // (the wave boxes are read from global memory: K1 has just written them, they sit in L2; staging them
    // in 96 KB of LDS was measured to cost more than it saved)
    __syncthreads();

    const double eps = (double)FLT_EPSILON;
    // one step of adoptBoundingBoxToPoint's loop: double the box, keeping the corner on the axes in `up`
    auto grow = [&](const bool up[3]) {
        double side = (double)(1u << s_depth) * P.res;
        for (int a = 0; a < 3; a++) {
            if (!up[a]) {
                s_mn[a] -= side;
                s_shift[a] += (long long)1 << s_depth;   // existing keys move up on this axis
            }
        }
        s_depth++;
        side = (double)(1u << s_depth) * P.res - eps;
        for (int a = 0; a < 3; a++) s_mx[a] = s_mn[a] + side;
        s_events++;
    };
    uint32_t range = 0;
    while (range < nranges) {
        // first range >= `range` whose box sticks out of the current octree box
        if (tid == 0) s_first = ~0ull;
        __syncthreads();
        {
            const double mn0 = s_mn[0], mn1 = s_mn[1], mn2 = s_mn[2], mx0 = s_mx[0], mx1 = s_mx[1], mx2 = s_mx[2];
            uint32_t mine = 0xffffffffu;
            for (uint32_t c = range + tid; c < nranges; c += 1024) {
                float b[6];
                for (int i = 0; i < 6; i++) b[i] = bboxes[(size_t)c * 6 + i];
                const bool viol = (double)b[0] < mn0 || (double)b[1] < mn1 || (double)b[2] < mn2 ||
                                  (double)b[3] >= mx0 || (double)b[4] >= mx1 || (double)b[5] >= mx2;
                if (viol) { mine = c; break; }
            }
            // one LDS atomic per wave, not per lane: after a growth step most ranges still stick out
            for (int off = 32; off > 0; off >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, off, 64));
            if ((tid & 63) == 0 && mine != 0xffffffffu) atomicMin(&s_first, (unsigned long long)mine);
        }
        __syncthreads();
        const unsigned long long hit = s_first;
        __syncthreads();
        if (hit == ~0ull) break;

        // Shortcut on the range's box: a point triggers growth when it violates the octree box, and the
        // step it takes depends only on the axes where it lies above the box.  If the range sticks out
        // below only, or above on exactly one axis and nowhere below, every triggering point of the range
        // has the same pattern, so the steps follow from the box of the range without reading its points.
        if (tid == 0) {
            float b[6];
            for (int i = 0; i < 6; i++) b[i] = bboxes[(size_t)hit * 6 + i];
            int resolved = 0;
            for (;;) {
                bool up[3], any_low = false;
                int n_up = 0;
                for (int a = 0; a < 3; a++) {
                    up[a] = (double)b[3 + a] >= s_mx[a];
                    n_up += up[a] ? 1 : 0;
                    any_low |= (double)b[a] < s_mn[a];
                }
                if (n_up == 0 && !any_low) { resolved = 1; break; }
                if (!(n_up == 0 || (n_up == 1 && !any_low))) break;   // mixed patterns: replay point by point
                if (s_depth >= 31) { atomicOr(&ctrl[C_ERR], ERR_DEPTH); resolved = 1; break; }
                grow(up);
            }
            s_resolved = resolved;
        }
        __syncthreads();
        if (s_resolved) {
            range = (uint32_t)hit + 1;
            continue;
        }

        // replay that range in index order, a tile of 4096 points at a time
        size_t r_lo = (size_t)hit * P.per_wave;
        size_t r_hi = r_lo + P.per_wave < P.n ? r_lo + P.per_wave : P.n;
        if (P.range_base_q != 0u) {
            r_lo = (size_t)range_first_step((uint32_t)hit, P.range_base_q, P.range_inc_q) * WAVE_STEP;
            r_hi = (size_t)range_first_step((uint32_t)hit + 1u, P.range_base_q, P.range_inc_q) * WAVE_STEP;
            r_lo = r_lo < P.n ? r_lo : P.n;
            r_hi = r_hi < P.n ? r_hi : P.n;
        }
        for (size_t tile = r_lo; tile < r_hi; tile += 4096) {
            const size_t base = tile + (size_t)tid * 4;
            float qx[4], qy[4], qz[4];
            for (int j = 0; j < 4; j++) {
                const bool ok = base + j < r_hi;
                qx[j] = ok ? x[base + j] : 0.f;
                qy[j] = ok ? y[base + j] : 0.f;
                qz[j] = ok ? z[base + j] : 0.f;
            }
            size_t from = tile;   // first index of this tile whose violation has not been handled yet
            for (;;) {
                if (tid == 0) s_first = ~0ull;
                __syncthreads();
                {
                    const double mn0 = s_mn[0], mn1 = s_mn[1], mn2 = s_mn[2], mx0 = s_mx[0], mx1 = s_mx[1], mx2 = s_mx[2];
                    unsigned long long mine = ~0ull;
                    for (int j = 0; j < 4; j++) {
                        const size_t idx = base + j;
                        if (idx < from || idx >= r_hi) continue;
                        if (!(isfinite(qx[j]) && isfinite(qy[j]) && isfinite(qz[j]))) continue;
                        const bool viol = (double)qx[j] < mn0 || (double)qy[j] < mn1 || (double)qz[j] < mn2 ||
                                          (double)qx[j] >= mx0 || (double)qy[j] >= mx1 || (double)qz[j] >= mx2;
                        if (viol) { mine = (unsigned long long)idx; break; }
                    }
                    // lanes hold ascending indices: the lowest lane with a violation has the wave's minimum
                    const unsigned long long vote = __ballot(mine != ~0ull);
                    if (vote != 0ull && (tid & 63) == __ffsll((long long)vote) - 1) atomicMin(&s_first, mine);
                }
                __syncthreads();
                const unsigned long long pidx = s_first;
                __syncthreads();
                if (pidx == ~0ull) break;
                if ((size_t)pidx >= base && (size_t)pidx < base + 4) {
                    // adoptBoundingBoxToPoint for this point: grow until it fits
                    const int j = (int)((size_t)pidx - base);
                    const double c[3] = {(double)(j == 0 ? qx[0] : j == 1 ? qx[1] : j == 2 ? qx[2] : qx[3]),
                                         (double)(j == 0 ? qy[0] : j == 1 ? qy[1] : j == 2 ? qy[2] : qy[3]),
                                         (double)(j == 0 ? qz[0] : j == 1 ? qz[1] : j == 2 ? qz[2] : qz[3])};
                    for (;;) {
                        bool up[3], any = false;
                        for (int a = 0; a < 3; a++) {
                            const bool lo = c[a] < s_mn[a];
                            up[a] = c[a] >= s_mx[a];
                            any |= lo | up[a];
                        }
                        if (!any) break;
                        if (s_depth >= 31) { atomicOr(&ctrl[C_ERR], ERR_DEPTH); break; }
                        grow(up);
                    }
                }
                from = (size_t)pidx + 1;
                __syncthreads();
            }
        }
        range = (uint32_t)hit + 1;
    }
    // the finalize pass orders leaves by the Morton code of their final keys: check here that it can
    // (depth, key range), so that it has no error of its own to report
    __syncthreads();
    {
        const int depth = s_depth;
        if (depth > 14) {
            if (tid == 0) atomicOr(&ctrl[C_ERR], ERR_DEPTH);
        } else {
            bool bad = false;
            for (uint32_t q = tid; q < leaf_cap; q += 1024) {
                const unsigned long long lp = leaf_keys[q];
                if (lp == 0ull) continue;
                for (int a = 0; a < 3; a++) {
                    const long long lk = (long long)unpack_leaf(lp, a) + s_shift[a];
                    bad |= lk < 0 || lk >= ((long long)1 << depth);
                }
            }
            if (bad) atomicOr(&ctrl[C_ERR], ERR_LEAF_RANGE);
        }
    }
    if (tid == 0) {
        ctrl[C_DEPTH] = (uint32_t)s_depth;
        ctrl[C_EVENTS] = (uint32_t)s_events;
        for (int a = 0; a < 3; a++) {
            ctrl[C_SHIFT + 2 * a] = (uint32_t)((unsigned long long)s_shift[a] & 0xffffffffu);
            ctrl[C_SHIFT + 2 * a + 1] = (uint32_t)((unsigned long long)s_shift[a] >> 32);
        }
    }
    __syncthreads();
    publish(ctrl, host_out, seq);
    zero_next_head();
}

// ---------------------------------------------------------------------------
// K3: output-order keys of the plain grid's sort path (index spaces beyond 2^28 cells)
// ---------------------------------------------------------------------------
// pcl::VoxelGrid's idx = i + j*div_x + k*div_x*div_y
__global__ void __launch_bounds__(256) make_sort_keys_kernel(VoxParams P, VoxWork W, uint32_t m, unsigned long long *__restrict__ sort_keys,
                                                            uint32_t *__restrict__ sort_vals) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    const uint32_t key = W.occupied[r];
    const uint32_t cell = key & ((1u << CELL_BITS) - 1), leaf_id = key >> CELL_BITS;
    const int c[3] = {(int)(cell % GRID_DIM), (int)((cell / GRID_DIM) % GRID_DIM), (int)(cell / (GRID_DIM * GRID_DIM))};
    const unsigned long long lp = W.leaf_keys[leaf_id];
    long long d[3];
    for (int a = 0; a < 3; a++) d[a] = (long long)(c[a] + P.ib[a] + 64 * unpack_leaf(lp, a) - 2) - (long long)(int)W.ctrl[C_MINB + a];
    const long long dx = (int)W.ctrl[C_DIVB], dy = (int)W.ctrl[C_DIVB + 1];
    sort_keys[r] = (unsigned long long)(d[0] + d[1] * dx + d[2] * dx * dy);
    sort_vals[r] = key;
}

// ---------------------------------------------------------------------------
// K4: emit in output order and clean the records
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) emit_and_clean_kernel(VoxParams P, VoxWork W, uint32_t m, const uint32_t *__restrict__ sorted_keys,
                                                            float *__restrict__ ox, float *__restrict__ oy, float *__restrict__ oz,
                                                            uint32_t *__restrict__ ow, int emit) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    const uint32_t key = emit ? sorted_keys[r] : W.occupied[r];
    ulonglong2 *rec = reinterpret_cast<ulonglong2 *>(record_ptr(W, key));
    if (emit) {
        const ulonglong2 w01 = rec[0], w23 = rec[1], w45 = rec[2], w67 = rec[3];
        const uint32_t cell = key & ((1u << CELL_BITS) - 1), leaf_id = key >> CELL_BITS;
        const int c[3] = {(int)(cell % GRID_DIM), (int)((cell / GRID_DIM) % GRID_DIM), (int)(cell / (GRID_DIM * GRID_DIM))};
        const unsigned long long lp = W.leaf_keys[leaf_id];
        double vox[3];
        for (int a = 0; a < 3; a++) vox[a] = (double)(c[a] + P.ib[a] + 64 * unpack_leaf(lp, a) - 2);
        const unsigned long long cr = w23.y, gb = w45.x;
        const uint32_t cnt = (uint32_t)(cr >> 32);
        const double scale = P.q_unit / (double)cnt;
        // mean = (voxel + mean position inside the voxel) / inv_leaf; one rounding to fp32 at the end
        ox[r] = (float)(vox[0] * P.vox_unit + (double)(long long)w01.x * scale);
        oy[r] = (float)(vox[1] * P.vox_unit + (double)(long long)w01.y * scale);
        oz[r] = (float)(vox[2] * P.vox_unit + (double)(long long)w23.x * scale);
        // pcl AccumulatorRGBA: float sums (exact integers here) / n, truncated
        const float fn = (float)cnt;
        const uint32_t rr = (uint32_t)__fdiv_rn((float)(uint32_t)(cr & 0xffffffffu), fn);
        const uint32_t gg = (uint32_t)__fdiv_rn((float)(uint32_t)(gb >> 32), fn);
        const uint32_t bb = (uint32_t)__fdiv_rn((float)(uint32_t)(gb & 0xffffffffu), fn);
        // tile: bits 0-3 / 4-7 as contribution counters, plus the OR word of the slow path
        uint32_t tile = (uint32_t)w67.y & 0xffu;
        for (int b = 0; b < 4; b++) {
            if ((w45.y >> (16 * b)) & 0xffffull) tile |= 1u << b;
            if ((w67.x >> (16 * b)) & 0xffffull) tile |= 16u << b;
        }
        ow[r] = (rr & 0xffu) | ((gg & 0xffu) << 8) | ((bb & 0xffu) << 16) | (tile << 24);
    }
    const ulonglong2 zero = {0ull, 0ull};
    rec[0] = zero; rec[1] = zero; rec[2] = zero; rec[3] = zero;
    const uint32_t bit_cell = key & ((1u << CELL_BITS) - 1);
    atomicAnd(&W.bitmaps[(size_t)(key >> CELL_BITS) * BITWORDS + (bit_cell >> 5)], ~(1u << (bit_cell & 31u)));
}

// ---------------------------------------------------------------------------
// Sort-free output order for the octree path: leaves in Morton order of their final keys,
// cells in ascending index inside a leaf = rank of a bit in the occupancy bitmaps.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void emit_record(const VoxParams &P, const VoxWork &W, unsigned long long lp, uint32_t key, uint32_t r,
                                            float *__restrict__ ox, float *__restrict__ oy, float *__restrict__ oz, uint32_t *__restrict__ ow) {
    ulonglong2 *rec = reinterpret_cast<ulonglong2 *>(record_ptr(W, key));
    const ulonglong2 w01 = rec[0], w23 = rec[1], w45 = rec[2], w67 = rec[3];
    const uint32_t cell = key & ((1u << CELL_BITS) - 1);
    const int c[3] = {(int)(cell % GRID_DIM), (int)((cell / GRID_DIM) % GRID_DIM), (int)(cell / (GRID_DIM * GRID_DIM))};
    double vox[3];
    for (int a = 0; a < 3; a++) vox[a] = (double)(c[a] + P.ib[a] + 64 * unpack_leaf(lp, a) - 2);
    const unsigned long long cr = w23.y, gb = w45.x;
    const uint32_t cnt = (uint32_t)(cr >> 32);
    // mean = voxel origin + mean offset (f64, one division), one rounding to fp32 at the end
    const double scale = P.q_unit / (double)cnt;
    ox[r] = (float)(vox[0] * P.vox_unit + (double)(long long)w01.x * scale);
    oy[r] = (float)(vox[1] * P.vox_unit + (double)(long long)w01.y * scale);
    oz[r] = (float)(vox[2] * P.vox_unit + (double)(long long)w23.x * scale);
    const float fn = (float)cnt;
    const uint32_t rr = (uint32_t)__fdiv_rn((float)(uint32_t)(cr & 0xffffffffu), fn);
    const uint32_t gg = (uint32_t)__fdiv_rn((float)(uint32_t)(gb >> 32), fn);
    const uint32_t bb = (uint32_t)__fdiv_rn((float)(uint32_t)(gb & 0xffffffffu), fn);
    uint32_t tile = (uint32_t)w67.y & 0xffu;
    for (int b = 0; b < 4; b++) {
        if ((w45.y >> (16 * b)) & 0xffffull) tile |= 1u << b;
        if ((w67.x >> (16 * b)) & 0xffffull) tile |= 16u << b;
    }
    ow[r] = (rr & 0xffu) | ((gg & 0xffu) << 8) | ((bb & 0xffu) << 16) | (tile << 24);
    const ulonglong2 zero = {0ull, 0ull};
    rec[0] = zero; rec[1] = zero; rec[2] = zero; rec[3] = zero;
}

// RANK_SEGS workgroups per leaf, each owning a contiguous slice of the leaf's bitmap: output base
// of the leaf (cells of all leaves that precede it in Morton order) + occupied cells in the
// earlier slices, ranks of the slice's cells from a popcount scan, then gather, emit and clean.
// Replaces the key sort: no pass over the outputs other than the emit itself.

// speculative != 0: launched before the host knows the outcome of the pass, into a result buffer sized from
// the previous call: the kernel takes the count from the control block and does nothing at all when the pass
// reported an error or the count exceeds `m_or_cap` (the host then runs it again, with the facts).
__global__ void __launch_bounds__(RANK_THREADS) rank_emit_kernel(VoxParams P, VoxWork W, uint32_t leaf_cap, uint32_t m_or_cap, int speculative,
                                                                 uint32_t *order, float *__restrict__ ox, float *__restrict__ oy,
                                                                 float *__restrict__ oz, uint32_t *__restrict__ ow) {
    // A workgroup's life is a chain of dependent memory round trips (it handles some sixty cells), so
    // everything that does not depend on loaded data is requested at once, up front: control words, this
    // leaf, every leaf's key and slice counts, the slice's bitmap words.  The cells in rank order go
    // through LDS, not through global memory (unless a slice has more than RANK_LDS_CELLS of them).
    constexpr uint32_t RANK_LDS_CELLS = 2048;
    __shared__ uint32_t wave_tot[RANK_THREADS / 64];
    __shared__ uint32_t s_cells[RANK_LDS_CELLS];
    const uint32_t p = blockIdx.x / RANK_SEGS, seg = blockIdx.x % RANK_SEGS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *bm = W.bitmaps + (size_t)p * BITWORDS;
    const int w_lo = (int)seg * SEG_WORDS;
    const int w_hi = min(w_lo + SEG_WORDS, BITWORDS);
    // ---- loads ----
    const uint32_t c_count = W.ctrl[C_COUNT], c_err = W.ctrl[C_ERR], c_depth = W.ctrl[C_DEPTH];
    uint32_t c_shift[6];
#pragma unroll
    for (int i = 0; i < 6; i++) c_shift[i] = W.ctrl[C_SHIFT + i];
    const unsigned long long lp = W.leaf_keys[p];
    uint32_t words[WORDS_PER_THREAD];
#pragma unroll
    for (int i = 0; i < WORDS_PER_THREAD; i++) {
        const int w = w_lo + threadIdx.x * WORDS_PER_THREAD + i;
        words[i] = bm[min(w, w_hi - 1)];
    }
    const uint32_t q0 = min((uint32_t)threadIdx.x, leaf_cap - 1u);   // this thread's leaf in the first round of the loop below
    const unsigned long long lq0 = W.leaf_keys[q0];
    uint4 sc0[RANK_SEGS / 4];
    {
        const uint4 *sc = reinterpret_cast<const uint4 *>(W.seg_count + (size_t)q0 * RANK_SEGS);
#pragma unroll
        for (int v = 0; v < RANK_SEGS / 4; v++) sc0[v] = sc[v];
    }
    const uint32_t own_earlier = threadIdx.x < seg ? W.seg_count[p * RANK_SEGS + threadIdx.x] : 0u;   // seg <= RANK_SEGS <= RANK_THREADS
    // ---- what they say ----
    uint32_t m = m_or_cap;
    if (speculative) {
        m = c_count;
        if (c_err != 0u || m > m_or_cap || m == 0u) return;
    }
    if (lp == 0ull) return;
    const int depth = (int)c_depth;
    long long shift[3];
    for (int a = 0; a < 3; a++) shift[a] = (long long)(((unsigned long long)c_shift[2 * a + 1] << 32) | c_shift[2 * a]);
    const auto morton = [&](unsigned long long leaf, unsigned long long &code) {
        long long lk[3];
        bool bad = false;
        for (int a = 0; a < 3; a++) {
            lk[a] = (long long)unpack_leaf(leaf, a) + shift[a];
            if (lk[a] < 0 || lk[a] >= ((long long)1 << depth)) bad = true;
        }
        code = 0;
        for (int b = depth - 1; b >= 0; b--) {
            code = (code << 3) | (((unsigned long long)(lk[0] >> b) & 1) << 2) | (((unsigned long long)(lk[1] >> b) & 1) << 1) |
                   ((unsigned long long)(lk[2] >> b) & 1);
        }
        return !bad;
    };
    unsigned long long mine;
    if (depth > 14 || !morton(lp, mine)) {
        if (threadIdx.x == 0) atomicOr(&W.ctrl[C_ERR], depth > 14 ? ERR_DEPTH : ERR_LEAF_RANGE);
        return;   // the host cleans up through the occupied list
    }
    // ---- base: cells of the leaves that come first, plus this leaf's cells in earlier slices ----
    uint32_t before = own_earlier;
    for (uint32_t q = threadIdx.x; q < leaf_cap; q += RANK_THREADS) {
        unsigned long long lq = lq0;
        uint4 scq[RANK_SEGS / 4];
#pragma unroll
        for (int v = 0; v < RANK_SEGS / 4; v++) scq[v] = sc0[v];
        if (q >= RANK_THREADS) {   // more leaves than threads (rare): the later rounds load as they go
            lq = W.leaf_keys[q];
            const uint4 *sc = reinterpret_cast<const uint4 *>(W.seg_count + (size_t)q * RANK_SEGS);
#pragma unroll
            for (int v = 0; v < RANK_SEGS / 4; v++) scq[v] = sc[v];
        }
        unsigned long long other;
        if (lq != 0ull && q != p && morton(lq, other) && other < mine) {
#pragma unroll
            for (int v = 0; v < RANK_SEGS / 4; v++) before += scq[v].x + scq[v].y + scq[v].z + scq[v].w;
        }
    }
    // (earlier slices may already have been cleaned by their own workgroups, so their cells are counted
    // from the per-slice totals K1 accumulated, not from the bitmaps)
    for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off, 64);
    // ---- ranks inside the slice: each lane owns WORDS_PER_THREAD consecutive bitmap words ----
    uint32_t mycount = 0;
#pragma unroll
    for (int i = 0; i < WORDS_PER_THREAD; i++) {
        const int w = w_lo + threadIdx.x * WORDS_PER_THREAD + i;
        if (w >= w_hi) words[i] = 0u;
        mycount += __popc(words[i]);
    }
    uint32_t inc = mycount;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    __shared__ uint32_t wave_cells[RANK_THREADS / 64];
    if (lane == 0) wave_tot[wave] = before;
    if (lane == 63) wave_cells[wave] = inc;
    __syncthreads();
    uint32_t base = 0, wbase = 0, total = 0;
    for (int w = 0; w < RANK_THREADS / 64; w++) {
        base += wave_tot[w];
        if (w < wave) wbase += wave_cells[w];
        total += wave_cells[w];
    }
    // phase 1: the slice's cells in rank order, the bitmap words cleaned
    uint32_t local = wbase + inc - mycount;
    if (base + total > m) {
        if (threadIdx.x == 0) atomicOr(&W.ctrl[C_ERR], ERR_LIST_FULL);
    }
    const bool in_lds = total <= RANK_LDS_CELLS;
#pragma unroll
    for (int i = 0; i < WORDS_PER_THREAD; i++) {
        uint32_t bits = words[i];
        const int w = w_lo + threadIdx.x * WORDS_PER_THREAD + i;
        if (bits) bm[w] = 0u;   // clean
        while (bits) {
            const int b = __ffs((int)bits) - 1;
            bits &= bits - 1;
            const uint32_t cell = (p << CELL_BITS) | (uint32_t)(w * 32 + b);
            if (in_lds) s_cells[local] = cell;
            else if (base + local < m) order[base + local] = cell;
            local++;
        }
    }
    __syncthreads();   // (this workgroup's order[] stores are visible to its own lanes from here on)
    // phase 2: gather, emit and clean, one cell per lane
    for (uint32_t i = threadIdx.x; i < total; i += RANK_THREADS) {
        const uint32_t r = base + i;
        if (r < m) emit_record(P, W, lp, in_lds ? s_cells[i] : __hip_atomic_load(&order[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), r, ox, oy, oz, ow);
    }
}

// ---------------------------------------------------------------------------
// Sort-free output order for the plain grid: pcl::VoxelGrid emits voxels by ascending
// idx = i + j * div_x + k * div_x * div_y.  A bitmap over that index space (it has at most 2^31
// cells by VoxelGrid's own rule; the bitmap path takes up to 2^28) turns the order into popcount ranks.
// ---------------------------------------------------------------------------
constexpr uint32_t GRID_BITMAP_MAX_CELLS = 1u << 28;
constexpr int GB_WORDS_PER_BLOCK = 1024;

__device__ __forceinline__ uint32_t voxelgrid_index(const VoxParams &P, const VoxWork &W, uint32_t key) {
    const uint32_t cell = key & ((1u << CELL_BITS) - 1), leaf_id = key >> CELL_BITS;
    const int c[3] = {(int)(cell % GRID_DIM), (int)((cell / GRID_DIM) % GRID_DIM), (int)(cell / (GRID_DIM * GRID_DIM))};
    const unsigned long long lp = W.leaf_keys[leaf_id];
    long long d[3];
    for (int a = 0; a < 3; a++) d[a] = (long long)(c[a] + P.ib[a] + 64 * unpack_leaf(lp, a) - 2) - (long long)(int)W.ctrl[C_MINB + a];
    const long long dx = (int)W.ctrl[C_DIVB], dy = (int)W.ctrl[C_DIVB + 1];
    return (uint32_t)(d[0] + d[1] * dx + d[2] * dx * dy);
}

// The five passes below can be launched before the host knows the outcome of the pass (right behind the replay
// kernel, like rank_emit_kernel on the octree path): they then take count and grid size from the control block
// and do nothing at all unless the pass succeeded and everything fits what the host provided for.
struct GridSpec {
    int on;                        // 0: m and nwords are the host's
    uint32_t m_cap;                // room in the result
    uint32_t words_cap;            // room in the index bitmap
    unsigned long long cells_max;  // largest index space the bitmap path takes
};
struct GridGate { uint32_t m, nwords; bool go; };
__device__ __forceinline__ GridGate grid_gate(const VoxWork &W, uint32_t m_host, uint32_t nwords_host, const GridSpec &spec) {
    if (!spec.on) return GridGate{m_host, nwords_host, true};
    const uint32_t m = W.ctrl[C_COUNT], err = W.ctrl[C_ERR];
    const unsigned long long cells = (unsigned long long)W.ctrl[C_DIVB] * W.ctrl[C_DIVB + 1] * W.ctrl[C_DIVB + 2];
    const unsigned long long nwords = (cells + 31) / 32;
    const bool go = err == 0u && m != 0u && m <= spec.m_cap && cells <= spec.cells_max && nwords <= spec.words_cap;
    return GridGate{m, (uint32_t)nwords, go};
}

// one bit per touched record; its index is kept for the passes that follow
__global__ void __launch_bounds__(256) grid_mark_kernel(VoxParams P, VoxWork W, uint32_t m_host, GridSpec spec, uint32_t *__restrict__ gbits,
                                                       uint32_t *__restrict__ gidx) {
    const GridGate gate = grid_gate(W, m_host, 0u, spec);
    if (!gate.go) return;
    const uint32_t m = gate.m;
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    const uint32_t idx = voxelgrid_index(P, W, W.occupied[r]);
    gidx[r] = idx;
    atomicOr(&gbits[idx >> 5], 1u << (idx & 31u));
}

// per block of 1024 bitmap words: set bits before each word (inside the block), set bits of the block
__global__ void __launch_bounds__(256) grid_block_kernel(VoxWork W, GridSpec spec, const uint32_t *__restrict__ gbits, uint32_t nwords_host,
                                                        uint32_t *__restrict__ word_prefix, uint32_t *__restrict__ block_sum) {
    __shared__ uint32_t wave_tot[4];
    const GridGate gate = grid_gate(W, 0u, nwords_host, spec);
    if (!gate.go) return;
    const uint32_t nwords = gate.nwords;
    if (blockIdx.x * (uint32_t)GB_WORDS_PER_BLOCK >= nwords) return;   // (a speculative launch covers the whole bitmap buffer)
    const uint32_t w0 = blockIdx.x * GB_WORDS_PER_BLOCK + threadIdx.x * 4;
    uint32_t c[4];
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        c[i] = w0 + i < nwords ? __popc(gbits[w0 + i]) : 0u;
        mine += c[i];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t before = inc - mine, total = 0;
    for (int w = 0; w < 4; w++) {
        if (w < wave) before += wave_tot[w];
        total += wave_tot[w];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (w0 + i < nwords) word_prefix[w0 + i] = before;
        before += c[i];
    }
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// exclusive scan of the block sums, one workgroup
__global__ void __launch_bounds__(1024) grid_blockscan_kernel(VoxWork W, GridSpec spec, uint32_t *__restrict__ block_sum, uint32_t nwords_host) {
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t carry;
    const GridGate gate = grid_gate(W, 0u, nwords_host, spec);
    if (!gate.go) return;
    const uint32_t nblocks = (gate.nwords + GB_WORDS_PER_BLOCK - 1) / GB_WORDS_PER_BLOCK;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < nblocks; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? block_sum[i] : 0;
        uint32_t inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        uint32_t wbase = 0;
        for (int w = 0; w < wave; w++) wbase += wave_tot[w];
        const uint32_t c = carry;
        if (i < nblocks) block_sum[i] = c + wbase + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + wbase + inc;
        __syncthreads();
    }
}

// rank of the record's bit = its output position; emit, clean the record and the leaf bitmap bit
__global__ void __launch_bounds__(256) grid_emit_kernel(VoxParams P, VoxWork W, uint32_t m_host, GridSpec spec, const uint32_t *__restrict__ gidx,
                                                       const uint32_t *__restrict__ gbits, const uint32_t *__restrict__ word_prefix,
                                                       const uint32_t *__restrict__ block_sum, float *__restrict__ ox, float *__restrict__ oy,
                                                       float *__restrict__ oz, uint32_t *__restrict__ ow) {
    const GridGate gate = grid_gate(W, m_host, 0u, spec);
    if (!gate.go) return;
    const uint32_t m = gate.m;
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    const uint32_t key = W.occupied[r], idx = gidx[r], w = idx >> 5;
    const uint32_t rank = block_sum[w / GB_WORDS_PER_BLOCK] + word_prefix[w] + __popc(gbits[w] & ((1u << (idx & 31u)) - 1u));
    if (rank < m) emit_record(P, W, W.leaf_keys[key >> CELL_BITS], key, rank, ox, oy, oz, ow);
    const uint32_t bit_cell = key & ((1u << CELL_BITS) - 1);
    atomicAnd(&W.bitmaps[(size_t)(key >> CELL_BITS) * BITWORDS + (bit_cell >> 5)], ~(1u << (bit_cell & 31u)));
}

// the index bitmap is left zeroed for the next call (after every rank has been read)
__global__ void __launch_bounds__(256) grid_unmark_kernel(VoxWork W, uint32_t m_host, GridSpec spec, const uint32_t *__restrict__ gidx,
                                                         uint32_t *__restrict__ gbits) {
    const GridGate gate = grid_gate(W, m_host, 0u, spec);
    if (!gate.go) return;
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r < gate.m) gbits[gidx[r] >> 5] = 0u;
}

// Error path of the octree variant (no list of touched records there): zero every record whose bit is
// set, and the bitmaps.  Same launch shape as rank_emit_kernel.
__global__ void __launch_bounds__(RANK_THREADS) clean_by_bitmap_kernel(VoxWork W) {
    const uint32_t p = blockIdx.x / RANK_SEGS, seg = blockIdx.x % RANK_SEGS;
    if (W.leaf_keys[p] == 0ull) return;
    uint32_t *bm = W.bitmaps + (size_t)p * BITWORDS;
    const int w_lo = (int)seg * SEG_WORDS, w_hi = min(w_lo + SEG_WORDS, BITWORDS);
    for (int w = w_lo + threadIdx.x; w < w_hi; w += RANK_THREADS) {
        uint32_t bits = bm[w];
        if (!bits) continue;
        bm[w] = 0u;
        while (bits) {
            const int b = __ffs((int)bits) - 1;
            bits &= bits - 1;
            ulonglong2 *rec = reinterpret_cast<ulonglong2 *>(record_ptr(W, (p << CELL_BITS) | (uint32_t)(w * 32 + b)));
            const ulonglong2 zero = {0ull, 0ull};
            rec[0] = zero; rec[1] = zero; rec[2] = zero; rec[3] = zero;
        }
    }
}

// The first point of a cloud the host has not seen (a filter result), once per cloud: one lane writes
// it into the pinned words (one launch instead of three copy operations).
__global__ void first_point_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, float *__restrict__ host_out) {
    host_out[0] = x[0]; host_out[1] = y[0]; host_out[2] = z[0];
}

// The first FINITE point (the octree skips the others, so it is the anchor): one workgroup walks the
// cloud from the front, 1024 points at a time, until a chunk holds one.  out = x, y, z, found.
__global__ void __launch_bounds__(1024) first_finite_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, size_t n,
                                                           float *__restrict__ host_out) {
    __shared__ unsigned long long s_first;
    for (size_t base = 0; base < n; base += 1024) {
        if (threadIdx.x == 0) s_first = ~0ull;
        __syncthreads();
        const size_t i = base + threadIdx.x;
        if (i < n && isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i])) atomicMin(&s_first, (unsigned long long)i);
        __syncthreads();
        const unsigned long long f = s_first;
        __syncthreads();
        if (f != ~0ull) {
            if (threadIdx.x == 0) { host_out[0] = x[f]; host_out[1] = y[f]; host_out[2] = z[f]; host_out[3] = 1.0f; }
            return;
        }
    }
    if (threadIdx.x == 0) host_out[3] = 0.0f;
}
