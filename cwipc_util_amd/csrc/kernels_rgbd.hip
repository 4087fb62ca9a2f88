// kernels_rgbd.hip -- gfx950 kernels of the RGB-D source (cwipc_hip_from_rgbd): every camera's depth and colour image in, one tiled
// cloud out, in camera order and row-major pixel order.  The per-pixel arithmetic is rgbd_terms.hpp's (float64, every operation
// rounded on its own); this file is the stable compaction around it: count -> scan -> scatter, one launch sequence for
// all cameras -- their pixels are numbered through and a workgroup owns TILE consecutive numbers, wherever camera borders fall.
//
// What is read.  The count pass reads the depth image, and of the rest only what an active filter looks at: no colour unless the green
// screen is on, and then only for pixels nothing else has dropped.  A depth pixel is one 16-bit load per lane, 128 contiguous bytes
// per wave.  A 3-byte colour pixel is NOT read as three byte loads: a lane reads the two aligned dwords that hold its bytes (the
// second is the next lane's first or in the same 64-byte line) and shifts the pixel out of the 64-bit pair -- two dword loads of
// 192 contiguous bytes per wave.  The host leaves 8 readable bytes behind every colour image for the last pixel's pair.
#include "internal.hpp"
#include "block_scan.hpp"

namespace cwipc_amd {
namespace k {

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int STEPS = 4;
constexpr int TILE = BLOCK * STEPS;           // pixels per workgroup: step s, lane t is pixel tile0 + s * BLOCK + t
constexpr uint32_t SMALL_FRAME = 262144;      // up to here the count kernel's last workgroup scans (the limit of kernels_basic.hip's flows)

// r | g << 8 | b << 16 of pixel p
__device__ __forceinline__ uint32_t load_colour(const uint8_t *__restrict__ colour, uint32_t p, uint32_t bpp) {
    if (bpp == 4u) {   // B, G, R, A
        const uint32_t w = ((const uint32_t *)colour)[p];
        return ((w >> 16) & 255u) | (w & 0xff00u) | ((w & 255u) << 16);
    }
    const size_t at = (size_t)p * 3u;
    const uint32_t *q = (const uint32_t *)(colour + (at & ~(size_t)3));
    const unsigned long long pair = (unsigned long long)q[0] | ((unsigned long long)q[1] << 32);
    return (uint32_t)(pair >> (8u * (unsigned)(at & 3u))) & 0xffffffu;   // R, G, B: already in that order
}

// the camera of pixel number g, searched upwards from k0 (the camera of the workgroup's first pixel)
__device__ __forceinline__ int camera_of(const RgbdCamDev *__restrict__ cams, int ncam, int k0, uint32_t g) {
    int k = k0;
    while (k + 1 < ncam && g >= cams[k + 1].first) k++;
    return k;
}

struct Pixel {
    int cam;
    int u, v;
    uint32_t p;   // its number inside its camera's image
    unsigned d;
};

// does pixel number g give a point?  px: what the scatter pass needs of it
__device__ __forceinline__ bool pixel_keep(const RgbdCamDev *__restrict__ cams, int ncam, int k0, uint32_t g, uint32_t total, const RgbdFilterTerms &f,
                                           unsigned active, Pixel &px) {
    if (g >= total) return false;
    px.cam = camera_of(cams, ncam, k0, g);
    const RgbdCamDev &c = cams[px.cam];
    px.p = g - c.first;
    px.d = c.depth[px.p];
    if (px.d == 0u) return false;
    px.v = (int)(px.p / c.width);
    px.u = (int)(px.p - (uint32_t)px.v * c.width);
    const uint8_t *colour = c.colour;
    const uint32_t p = px.p, bpp = c.bpp;
    return rgbd_keep(c.t, f, active, px.u, px.v, px.d, [=]() { return load_colour(colour, p, bpp); });
}

// the workgroup's count (thread 0's return value)
__device__ __forceinline__ uint32_t count_tile(const RgbdCamDev *__restrict__ cams, int ncam, uint32_t total, const RgbdFilterTerms &f, unsigned active,
                                               uint32_t *wave_sum) {
    const uint32_t tile0 = blockIdx.x * (uint32_t)TILE;
    const int k0 = camera_of(cams, ncam, 0, tile0);
    uint32_t cnt = 0;
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
        Pixel px;
        const bool keep = pixel_keep(cams, ncam, k0, tile0 + (uint32_t)(s * BLOCK) + threadIdx.x, total, f, active, px);
        cnt += (uint32_t)__popcll(__ballot(keep));   // (every lane of the wave holds the wave's count)
    }
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    uint32_t t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < WAVES; w++) t += wave_sum[w];
    return t;
}

__global__ void __launch_bounds__(BLOCK) rgbd_count_kernel(const RgbdCamDev *__restrict__ cams, int ncam, uint32_t total, RgbdFilterTerms f, unsigned active,
                                                          uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_sum[WAVES];
    const uint32_t t = count_tile(cams, ncam, total, f, active, wave_sum);
    if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

// count and scan in one launch: compact_count_scan_kernel's ticket (kernels_basic.hip)
__global__ void __launch_bounds__(BLOCK) rgbd_count_scan_kernel(const RgbdCamDev *__restrict__ cams, int ncam, uint32_t total, RgbdFilterTerms f,
                                                               unsigned active, uint32_t *__restrict__ counts, uint32_t *__restrict__ ticket,
                                                               unsigned long long *__restrict__ total_host, uint32_t tag) {
    __shared__ uint32_t wave_sum[WAVES];
    __shared__ uint32_t is_last;
    const uint32_t t = count_tile(cams, ncam, total, f, active, wave_sum);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&counts[blockIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t before = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        is_last = before == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next kernel that uses it
    scan_block_counts<BLOCK>(counts, gridDim.x, total_host, tag);
}

// offsets: the scanned counts.  A kept pixel's rank inside the tile: the kept pixels of the steps before its own, of the waves before
// its own in its step, and of the lanes before its own in its wave -- pixel order.
__global__ void __launch_bounds__(BLOCK) rgbd_scatter_kernel(const RgbdCamDev *__restrict__ cams, int ncam, uint32_t total, RgbdFilterTerms f, unsigned active,
                                                            const uint32_t *__restrict__ offsets, float *__restrict__ ox, float *__restrict__ oy,
                                                            float *__restrict__ oz, uint32_t *__restrict__ ow) {
    __shared__ uint32_t wave_sum[STEPS][WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t tile0 = blockIdx.x * (uint32_t)TILE;
    const int k0 = camera_of(cams, ncam, 0, tile0);
    Pixel px[STEPS];
    bool keep[STEPS];
    uint32_t before_lane[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
        keep[s] = pixel_keep(cams, ncam, k0, tile0 + (uint32_t)(s * BLOCK) + threadIdx.x, total, f, active, px[s]);
        const unsigned long long ballot = __ballot(keep[s]);
        before_lane[s] = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) wave_sum[s][wave] = (uint32_t)__popcll(ballot);
    }
    __syncthreads();
    uint32_t at = offsets[blockIdx.x];
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
        uint32_t before_wave = 0, step_total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint32_t n = wave_sum[s][w];
            if (w < wave) before_wave += n;
            step_total += n;
        }
        if (keep[s]) {
            const uint32_t idx = at + before_wave + before_lane[s];
            const RgbdCamDev &c = cams[px[s].cam];
            float pt[3];
            rgbd_point(c.t, px[s].u, px[s].v, px[s].d, pt);
            const uint32_t w = load_colour(c.colour, px[s].p, c.bpp) | (c.tile << 24);
            if (idx < total) {   // (always, the two passes seeing the same images; no store past the planes whatever happens)
                ox[idx] = pt[0]; oy[idx] = pt[1]; oz[idx] = pt[2]; ow[idx] = w;
            }
        }
        at += step_total;
    }
}

}  // namespace

size_t rgbd_blocks(uint32_t total_pixels) { return ((size_t)total_pixels + TILE - 1) / TILE; }

void rgbd_count(const RgbdCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, uint32_t *counts, uint32_t *ticket,
                unsigned long long *total_host, uint32_t tag, hipStream_t s) {
    const size_t nb = rgbd_blocks(total_pixels);
    const unsigned active = rgbd_active(f);
    if (total_pixels <= SMALL_FRAME && ticket) {
        CW_LAUNCH("rgbd_count", rgbd_count_scan_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, s, cams, ncam, total_pixels, f, active, counts, ticket, total_host,
                  tag);
    } else {
        CW_LAUNCH("rgbd_count", rgbd_count_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, s, cams, ncam, total_pixels, f, active, counts);
        compact_scan(counts, nb, total_host, tag, s);
    }
}

void rgbd_scatter(const RgbdCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, const uint32_t *offsets, const DeviceSoA &dst,
                  hipStream_t s) {
    CW_LAUNCH("rgbd_scatter", rgbd_scatter_kernel, dim3((unsigned)rgbd_blocks(total_pixels)), dim3(BLOCK), 0, s, cams, ncam, total_pixels, f, rgbd_active(f),
              offsets, dst.x(), dst.y(), dst.z(), dst.rgbt());
}

}  // namespace k
}  // namespace cwipc_amd
