// kernels_render.hip -- gfx950 kernels of cwipc_hip_render: a cloud and a pinhole view in, a colour image, a depth image and a
// per-pixel point index out (the step the reference's MultiCameraCoarseAruco._find_markers does with an open3d window,
// python/cwipc/registration/multicoarse.py:333-360: look at a camera's tile from the origin, grab colour and depth).
//
// The contract (include/cwipc_util_amd/hip_ext.h has it in full; tests/render_model.py is its numpy model).  Every operation is
// rounded on its own (the build passes -ffp-contract=off), E = the view's extrinsic:
//   a point takes part iff (tilemask == 0 || (tile & tilemask) != 0) and x, y, z are finite;
//   xc = ((E00*x + E01*y) + E02*z) + E03 in f64 from the float32 coordinates (yc, zc alike); dropped unless near < zc < far;
//   u = fx*(xc/zc) + cx, v = fy*(yc/zc) + cy; col = floor(u), row = floor(v); dropped unless -(h+1) < floor(u) < width+h and the same
//   for v, h = (point_size-1)/2, decided in f64: no float is turned into an integer before it is known to fit;
//   the splat is every pixel of the image with |c-col| <= h and |r-row| <= h; a pixel goes to the smallest (float)zc, among equal
//   depths to the smallest point index.
//
// The z-buffer is one 64-bit key per pixel, float_bits((float)zc) << 32 | index: zc > near > 0, so the depth is a positive float and
// positive floats order as their bit patterns do; the index in the low word breaks ties.  All ones = nothing yet (no point has the
// index 0xFFFFFFFF).  Three kernels: fill the keys, one lane per point taking the minimum into the keys of its splat, one lane per
// four pixels unpacking the winners.  The minimum of a set does not depend on the order its members arrive in: the same input
// gives the same bytes.
#include "internal.hpp"
#include "block_scan.hpp"

#include <cmath>

namespace cwipc_amd {
namespace k {

static constexpr int RBLOCK = 256;
static constexpr unsigned long long RENDER_EMPTY = ~0ull;

static inline unsigned render_grid(size_t items) {
    size_t g = (items + RBLOCK - 1) / RBLOCK;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;   // grid-stride beyond eight workgroups per CU
    return (unsigned)g;
}

// keys[0, npix) = all ones, 16 bytes per lane and step; *covered = 0 (the resolve kernel counts into it)
__global__ void __launch_bounds__(RBLOCK) render_fill_kernel(unsigned long long *__restrict__ keys, size_t npix, uint32_t *__restrict__ covered) {
    const size_t stride = (size_t)gridDim.x * RBLOCK;
    const size_t npairs = npix / 2;
    for (size_t i = (size_t)blockIdx.x * RBLOCK + threadIdx.x; i < npairs; i += stride)
        reinterpret_cast<ulonglong2 *>(keys)[i] = make_ulonglong2(RENDER_EMPTY, RENDER_EMPTY);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (npix & 1) keys[npix - 1] = RENDER_EMPTY;
        *covered = 0;
    }
}

// One lane per point.  In front of every atomic a relaxed load: keys only ever decrease, so a key that is already smaller than
// this point's stays smaller and the atomic can be left out (a stale, larger value only costs an atomic that changes nothing).
// In a dense cloud most pixels have their winner early, and an atomic drops its line from the XCD's L2 while a load does not.
__global__ void __launch_bounds__(RBLOCK) render_splat_kernel(RenderArgs a, const float *__restrict__ x, const float *__restrict__ y,
                                                             const float *__restrict__ z, const uint32_t *__restrict__ rgbt, size_t n,
                                                             unsigned long long *__restrict__ keys) {
    const size_t stride = (size_t)gridDim.x * RBLOCK;
    const int h = a.half;
    for (size_t i = (size_t)blockIdx.x * RBLOCK + threadIdx.x; i < n; i += stride) {
        if (a.tilemask != 0 && ((int)(rgbt[i] >> 24) & a.tilemask) == 0) continue;
        const float fx = x[i], fy = y[i], fz = z[i];
        if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) continue;
        const double px = (double)fx, py = (double)fy, pz = (double)fz;
        const double zc = ((a.e[8] * px + a.e[9] * py) + a.e[10] * pz) + a.e[11];
        if (!(a.near_z < zc && zc < a.far_z)) continue;   // (false for a NaN too)
        const double xc = ((a.e[0] * px + a.e[1] * py) + a.e[2] * pz) + a.e[3];
        const double yc = ((a.e[4] * px + a.e[5] * py) + a.e[6] * pz) + a.e[7];
        const double fu = floor(a.fx * (xc / zc) + a.cx);
        const double fv = floor(a.fy * (yc / zc) + a.cy);
        // can the splat touch the image?  In f64: only a value that passes is small enough for an int (false for NaN and +-inf)
        if (!(-(double)(h + 1) < fu && fu < (double)(a.width + h) && -(double)(h + 1) < fv && fv < (double)(a.height + h))) continue;
        const int col = (int)fu, row = (int)fv;   // col in [-h, width + h), row in [-h, height + h)
        const unsigned long long key = ((unsigned long long)__float_as_uint((float)zc) << 32) | (unsigned long long)(uint32_t)i;
        const int c0 = col - h < 0 ? 0 : col - h, c1 = col + h > a.width - 1 ? a.width - 1 : col + h;
        const int r0 = row - h < 0 ? 0 : row - h, r1 = row + h > a.height - 1 ? a.height - 1 : row + h;
        for (int r = r0; r <= r1; r++) {
            unsigned long long *line = keys + (size_t)r * (size_t)a.width;   // r in [0, height), c in [0, width): inside the key buffer
            for (int c = c0; c <= c1; c++) {
                if (__hip_atomic_load(line + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key)
                    (void)__hip_atomic_fetch_min(line + c, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// One lane per four pixels: 32 bytes of keys in, 16 bytes of depth, 16 of index and 12 of colour out.  rgb: r, g, b per pixel, i.e.
// the low three bytes of the winner's rgbt word in memory order.
__global__ void __launch_bounds__(RBLOCK) render_resolve_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ rgbt, size_t npix,
                                                               uint32_t background, float *__restrict__ depth, uint8_t *__restrict__ rgb,
                                                               int32_t *__restrict__ index /* may be nullptr */, uint32_t *__restrict__ covered) {
    const size_t stride = (size_t)gridDim.x * RBLOCK;
    const size_t ngroups = (npix + 3) / 4;
    uint32_t mine = 0;
    for (size_t g = (size_t)blockIdx.x * RBLOCK + threadIdx.x; g < ngroups; g += stride) {
        const size_t base = g * 4;
        const bool full = base + 4 <= npix;
        unsigned long long kk[4];
        if (full) {
            const ulonglong2 lo = reinterpret_cast<const ulonglong2 *>(keys + base)[0], hi = reinterpret_cast<const ulonglong2 *>(keys + base)[1];
            kk[0] = lo.x; kk[1] = lo.y; kk[2] = hi.x; kk[3] = hi.y;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) kk[j] = base + j < npix ? keys[base + j] : RENDER_EMPTY;
        }
        float d[4];
        int32_t ix[4];
        uint32_t col[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (kk[j] == RENDER_EMPTY) {
                d[j] = 0.0f; ix[j] = -1; col[j] = background;
            } else {
                const uint32_t who = (uint32_t)kk[j];
                d[j] = __uint_as_float((uint32_t)(kk[j] >> 32));
                ix[j] = (int32_t)who;
                col[j] = rgbt[who] & 0x00FFFFFFu;
                mine++;
            }
        }
        if (full) {
            reinterpret_cast<float4 *>(depth + base)[0] = make_float4(d[0], d[1], d[2], d[3]);
            if (index) reinterpret_cast<int4 *>(index + base)[0] = make_int4(ix[0], ix[1], ix[2], ix[3]);
            uint32_t *w = reinterpret_cast<uint32_t *>(rgb + base * 3);   // 12 g bytes into a 16-byte aligned buffer
            w[0] = col[0] | (col[1] << 24);
            w[1] = (col[1] >> 8) | (col[2] << 16);
            w[2] = (col[2] >> 16) | (col[3] << 8);
        } else {
            for (int j = 0; j < 4 && base + j < npix; j++) {
                depth[base + j] = d[j];
                if (index) index[base + j] = ix[j];
                rgb[(base + j) * 3 + 0] = (uint8_t)col[j];
                rgb[(base + j) * 3 + 1] = (uint8_t)(col[j] >> 8);
                rgb[(base + j) * 3 + 2] = (uint8_t)(col[j] >> 16);
            }
        }
    }
    wave_reduce_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(covered, mine);
}

void render_fill(unsigned long long *keys, size_t npix, uint32_t *covered, hipStream_t s) {
    CW_LAUNCH("render_fill", render_fill_kernel, dim3(render_grid(npix / 2)), dim3(RBLOCK), 0, s, keys, npix, covered);
}

void render_splat(const DeviceSoA &src, const RenderArgs &a, unsigned long long *keys, hipStream_t s) {
    if (!src.npoints) return;
    CW_LAUNCH("render_splat", render_splat_kernel, dim3(render_grid(src.npoints)), dim3(RBLOCK), 0, s, a, src.x(), src.y(), src.z(), src.rgbt(), src.npoints, keys);
}

void render_resolve(const unsigned long long *keys, const uint32_t *rgbt, size_t npix, uint32_t background, float *depth, uint8_t *rgb, int32_t *index,
                    uint32_t *covered, hipStream_t s) {
    CW_LAUNCH("render_resolve", render_resolve_kernel, dim3(render_grid((npix + 3) / 4)), dim3(RBLOCK), 0, s, keys, rgbt, npix, background, depth, rgb, index,
              covered);
}

}  // namespace k
}  // namespace cwipc_amd
