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
//
// The raw entry (cwipc_hip_rgbd_rig_grab, rgbd_lens.hpp) runs up to three kernels in front of the same count -> scan -> scatter: the
// depth erosion as two passes over one 1-bit validity plane (a wave's 64 pixels of a row are one ballot word), and the registration,
// which gives every depth pixel the colour pixel its point projects to and clears the depth of those that have none (on request also
// of those the colour camera cannot see: a z-buffer of the colour grid, filled by rgbd_zsplat in front of it).  After it the
// frame is a depth image with an aligned RGB8 image again; count and scatter are the kernels above instantiated for a camera type
// that also knows its ray table (Cam = RgbdRawCamDev), the existing instantiation (Cam = RgbdCamDev) computing what it always did.
// On request (cwipc_hip_rgbd_rig_grab_filtered, rgbd_depthfilter.hpp) the depth post-processing runs in front of the erosion: the
// spatial filter's line passes, one lane per row or column walking it in LDS, and the temporal filter's per-pixel update of the image
// and of the state the rig keeps from grab to grab.  A decimated rig (cwipc_hip_rgbd_rig_create_decimated, rgbd_decimate.hpp) runs
// rgbd_decimate in front of all of it, full-size depth images in, the rig's grid out; cwipc_hip_rgbd_rig_grab_filled fills holes
// between the temporal filter and the erosion, along rows as a wave scan or from a pixel's eight neighbours.
#include "internal.hpp"
#include "block_scan.hpp"

#include <type_traits>

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
template <class Cam>
__device__ __forceinline__ int camera_of(const Cam *__restrict__ cams, int ncam, int k0, uint32_t g) {
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
template <class Cam>
__device__ __forceinline__ bool pixel_keep(const Cam *__restrict__ cams, int ncam, int k0, uint32_t g, uint32_t total, const RgbdFilterTerms &f,
                                           unsigned active, Pixel &px) {
    if (g >= total) return false;
    px.cam = camera_of(cams, ncam, k0, g);
    const Cam &c = cams[px.cam];
    px.p = g - c.first;
    px.d = c.depth[px.p];
    if (px.d == 0u) return false;
    px.v = (int)(px.p / c.width);
    px.u = (int)(px.p - (uint32_t)px.v * c.width);
    const uint8_t *colour = c.colour;
    const uint32_t p = px.p, bpp = c.bpp;
    if constexpr (std::is_same<Cam, RgbdRawCamDev>::value) {
        if (c.rays) return rgbd_keep_ray(c.t, f, active, c.rays + 2 * (size_t)p, px.d, [=]() { return load_colour(colour, p, bpp); });
    }
    return rgbd_keep(c.t, f, active, px.u, px.v, px.d, [=]() { return load_colour(colour, p, bpp); });
}

// the workgroup's count (thread 0's return value)
template <class Cam>
__device__ __forceinline__ uint32_t count_tile(const Cam *__restrict__ cams, int ncam, uint32_t total, const RgbdFilterTerms &f, unsigned active,
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

template <class Cam>
__global__ void __launch_bounds__(BLOCK) rgbd_count_kernel(const Cam *__restrict__ cams, int ncam, uint32_t total, RgbdFilterTerms f, unsigned active,
                                                          uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_sum[WAVES];
    const uint32_t t = count_tile(cams, ncam, total, f, active, wave_sum);
    if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

// count and scan in one launch (last_block_scans, block_scan.hpp)
template <class Cam>
__global__ void __launch_bounds__(BLOCK) rgbd_count_scan_kernel(const Cam *__restrict__ cams, int ncam, uint32_t total, RgbdFilterTerms f,
                                                               unsigned active, uint32_t *__restrict__ counts, uint32_t *__restrict__ ticket,
                                                               unsigned long long *__restrict__ total_host, uint32_t tag) {
    __shared__ uint32_t wave_sum[WAVES];
    last_block_scans<BLOCK>(count_tile(cams, ncam, total, f, active, wave_sum), counts, ticket, total_host, tag);
}

// offsets: the scanned counts.  A kept pixel's rank inside the tile: the kept pixels of the steps before its own, of the waves before
// its own in its step, and of the lanes before its own in its wave -- pixel order.
template <class Cam>
__global__ void __launch_bounds__(BLOCK) rgbd_scatter_kernel(const Cam *__restrict__ cams, int ncam, uint32_t total, RgbdFilterTerms f, unsigned active,
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
            const Cam &c = cams[px[s].cam];
            float pt[3];
            if constexpr (std::is_same<Cam, RgbdRawCamDev>::value)
                rgbd_raw_point(c.t, c.rays ? c.rays + 2 * (size_t)px[s].p : nullptr, px[s].u, px[s].v, px[s].d, pt);
            else
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

namespace {

template <class Cam>
void count_launch(const Cam *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, uint32_t *counts, uint32_t *ticket,
                  unsigned long long *total_host, uint32_t tag, hipStream_t s) {
    const size_t nb = rgbd_blocks(total_pixels);
    const unsigned active = rgbd_active(f);
    if (total_pixels <= SMALL_FRAME && ticket) {
        CW_LAUNCH("rgbd_count", rgbd_count_scan_kernel<Cam>, dim3((unsigned)nb), dim3(BLOCK), 0, s, cams, ncam, total_pixels, f, active, counts, ticket,
                  total_host, tag);
    } else {
        CW_LAUNCH("rgbd_count", rgbd_count_kernel<Cam>, dim3((unsigned)nb), dim3(BLOCK), 0, s, cams, ncam, total_pixels, f, active, counts);
        compact_scan(counts, nb, total_host, tag, s);
    }
}

template <class Cam>
void scatter_launch(const Cam *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, const uint32_t *offsets, const DeviceSoA &dst, hipStream_t s) {
    CW_LAUNCH("rgbd_scatter", rgbd_scatter_kernel<Cam>, dim3((unsigned)rgbd_blocks(total_pixels)), dim3(BLOCK), 0, s, cams, ncam, total_pixels, f,
              rgbd_active(f), offsets, dst.x(), dst.y(), dst.z(), dst.rgbt());
}

// ---- the raw entry's own kernels ----

// ---- the depth post-processing (rgbd_depthfilter.hpp), in front of the erosion ----
//
// A line of the spatial filter is a chain of dependent float64 steps, so a frame's parallelism is its number of lines.  One workgroup
// is one wave and owns LINES neighbouring lines of one camera -- rows in the row kernel, columns in the column kernel -- which it holds
// in LDS as they lie in the image: it loads them coalesced (every lane along a row), lane l < LINES then walks line l forward and
// backward with the running value in a register (tile_walk: the pixels go through registers eight at a time), and the lines are
// stored coalesced.  A line of up to LINE_CHUNK pixels is loaded and stored once for its two passes.  A longer one goes through LDS
// in chunks: forward chunk by chunk with a store each, then backward over the chunks in reverse, the running value carried from chunk
// to chunk -- the line is NOT cut, the order of its steps is the rule's.  Which lines share a workgroup changes nothing: a lane
// touches only its own line's pixels between two barriers.  Measured: a launch lasts as long as one line's chain, about
// 0.1 us per pixel and pass, which is the step's instructions issued by one wave, not memory.
constexpr int LINES = 32;
constexpr int LINE_CHUNK = 1020;
constexpr int ROW_STRIDE = LINE_CHUNK + 2;    // of a row kernel's tile, in pixels: 511 dwords, odd, so the lanes' walks fall on different banks

uint32_t line_groups(uint32_t lines) { return (lines + LINES - 1) / LINES; }

// ROWS: the tile is nlines rows of np pixels from column p0 on, tile[r * ROW_STRIDE + i]; columns: np rows (from row p0 on) of nlines
// pixels, tile[i * LINES + c].  Either way `line` is the line's number in the tile and i the position along it.
template <bool ROWS>
__device__ __forceinline__ uint32_t tile_at(uint32_t line, uint32_t i) {
    return ROWS ? line * (uint32_t)ROW_STRIDE + i : i * (uint32_t)LINES + line;
}

// global <-> LDS, coalesced along the image's rows.  line0 + nlines and p0 + np are inside the image (the caller's minima).
template <bool ROWS, bool STORE>
__device__ __forceinline__ void tile_copy(uint16_t *__restrict__ image, uint32_t width, uint32_t line0, uint32_t nlines, uint32_t p0, uint32_t np,
                                          uint16_t *tile) {
    const uint32_t lane = threadIdx.x;
    if (ROWS) {
        for (uint32_t r = 0; r < nlines; r++) {
            uint16_t *row = image + (size_t)(line0 + r) * width + p0;
            for (uint32_t i = lane; i < np; i += 64u) {
                if (STORE) row[i] = tile[tile_at<true>(r, i)];
                else tile[tile_at<true>(r, i)] = row[i];
            }
        }
    } else {
        // two rows per step: lanes 0 .. 31 the even one, lanes 32 .. 63 the odd one
        const uint32_t c = lane & 31u;
        if (c < nlines)
            for (uint32_t i = lane >> 5; i < np; i += 2u) {
                uint16_t *at = image + (size_t)(p0 + i) * width + line0 + c;
                if (STORE) *at = tile[tile_at<false>(c, i)];
                else tile[tile_at<false>(c, i)] = *at;
            }
    }
}

// One pass of lane `line` over the np pixels of its line that are in the tile, in pass order.  The chain of steps does not wait for
// LDS: the pixels go through registers eight at a time, the next eight being read while these are walked.
template <bool ROWS, bool BACKWARD>
__device__ __forceinline__ void tile_walk(const RgbdSmoothTerms &t, double &s, uint16_t *tile, uint32_t line, uint32_t np) {
    constexpr uint32_t B = 8;
    const auto at = [=](uint32_t i) { return tile_at<ROWS>(line, BACKWARD ? np - 1u - i : i); };   // (i < np)
    const uint32_t full = np - np % B;
    uint16_t cur[B], nxt[B];
    if (full) {
#pragma unroll
        for (uint32_t j = 0; j < B; j++) cur[j] = tile[at(j)];
    }
    for (uint32_t i0 = 0; i0 < full; i0 += B) {
        const bool more = i0 + B < full;
        if (more) {
#pragma unroll
            for (uint32_t j = 0; j < B; j++) nxt[j] = tile[at(i0 + B + j)];
        }
#pragma unroll
        for (uint32_t j = 0; j < B; j++) rgbd_line_step(t, s, cur[j]);
#pragma unroll
        for (uint32_t j = 0; j < B; j++) tile[at(i0 + j)] = cur[j];
        if (more) {
#pragma unroll
            for (uint32_t j = 0; j < B; j++) cur[j] = nxt[j];
        }
    }
    for (uint32_t i = full; i < np; i++) rgbd_line_step(t, s, tile[at(i)]);
}

template <bool ROWS>
__global__ void __launch_bounds__(64) rgbd_spatial_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam, RgbdSmoothTerms t) {
    __shared__ uint16_t tile[LINES * ROW_STRIDE];
    // the camera of this line group and the group's number in it
    uint32_t group = blockIdx.x;
    int k = 0;
    for (; k < ncam; k++) {
        const uint32_t n = ((ROWS ? cams[k].height : cams[k].width) + (uint32_t)LINES - 1u) / (uint32_t)LINES;
        if (group < n) break;
        group -= n;
    }
    if (k == ncam) return;   // (the whole workgroup; the host launches exactly the groups there are)
    const RgbdRawCamDev &c = cams[k];
    const uint32_t width = c.width, nline_all = ROWS ? c.height : c.width, n = ROWS ? c.width : c.height;
    const uint32_t line0 = group * (uint32_t)LINES, nlines = nline_all - line0 < (uint32_t)LINES ? nline_all - line0 : (uint32_t)LINES;
    const uint32_t nchunks = (n + (uint32_t)LINE_CHUNK - 1u) / (uint32_t)LINE_CHUNK;
    const uint32_t lane = threadIdx.x;
    double s = 0.0;   // (0 in front of a pass's first pixel: it takes over that pixel's value, rgbd_depthfilter.hpp)
    for (uint32_t ch = 0; ch < nchunks; ch++) {
        const uint32_t p0 = ch * (uint32_t)LINE_CHUNK, np = n - p0 < (uint32_t)LINE_CHUNK ? n - p0 : (uint32_t)LINE_CHUNK;
        tile_copy<ROWS, false>(c.depth_rw, width, line0, nlines, p0, np, tile);
        __syncthreads();
        if (lane < nlines) tile_walk<ROWS, false>(t, s, tile, lane, np);
        __syncthreads();
        if (nchunks > 1u) {
            tile_copy<ROWS, true>(c.depth_rw, width, line0, nlines, p0, np, tile);
            __syncthreads();   // (the next load overwrites the tile, and may read what other lanes stored)
        }
    }
    s = 0.0;
    for (uint32_t ch = nchunks; ch-- > 0u;) {
        const uint32_t p0 = ch * (uint32_t)LINE_CHUNK, np = n - p0 < (uint32_t)LINE_CHUNK ? n - p0 : (uint32_t)LINE_CHUNK;
        if (nchunks > 1u) {
            tile_copy<ROWS, false>(c.depth_rw, width, line0, nlines, p0, np, tile);
            __syncthreads();
        }
        if (lane < nlines) tile_walk<ROWS, true>(t, s, tile, lane, np);
        __syncthreads();
        tile_copy<ROWS, true>(c.depth_rw, width, line0, nlines, p0, np, tile);
        __syncthreads();
    }
}

// The temporal filter: one lane per depth pixel of the frame, whose state entry has the pixel's number.
__global__ void __launch_bounds__(BLOCK) rgbd_temporal_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam, uint32_t total, RgbdSmoothTerms t,
                                                             int persistency, double *__restrict__ value, uint8_t *__restrict__ history) {
    const uint32_t g = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
    if (g >= total) return;
    const RgbdRawCamDev &c = cams[camera_of(cams, ncam, 0, g)];
    const uint32_t p = g - c.first;
    double s = value[g];
    uint8_t h = history[g];
    c.depth_rw[p] = rgbd_temporal_step(t, persistency, c.depth_rw[p], s, h);
    value[g] = s;
    history[g] = h;
}

// the camera of validity word g
__device__ __forceinline__ int camera_of_word(const RgbdRawCamDev *__restrict__ cams, int ncam, uint32_t g) {
    int k = 0;
    while (k + 1 < ncam && g >= cams[k + 1].wfirst) k++;
    return k;
}

// Erosion, the row pass.  Wave g owns word g of the word grid: camera after camera, row after row, ceil(width / 64) words per row.
// Its 64 pixels' validity is one ballot; so is either neighbour's (all ones where the row ends: outside the image nothing erodes).
__global__ void __launch_bounds__(BLOCK) rgbd_erode_rows_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam, uint32_t total_words, int ex,
                                                               unsigned long long *__restrict__ words) {
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * (uint32_t)WAVES + (threadIdx.x >> 6);
    if (g >= total_words) return;   // (the whole wave)
    const RgbdRawCamDev &c = cams[camera_of_word(cams, ncam, g)];
    const uint32_t local = g - c.wfirst, row = local / c.wpr, wi = local - row * c.wpr;
    const uint16_t *__restrict__ line = c.depth + (size_t)row * c.width;
    const uint32_t u = wi * 64u + (uint32_t)lane;
    const unsigned long long own = __ballot(u >= c.width || line[u] != 0);
    unsigned long long left = ~0ull, right = ~0ull;
    if (ex > 0) {
        if (wi > 0) left = __ballot(line[u - 64u] != 0);   // (a whole word: all its pixels are in the row)
        if (wi + 1 < c.wpr) right = __ballot(u + 64u >= c.width || line[u + 64u] != 0);
    }
    const unsigned long long acc = rgbd_erode_word(left, own, right, ex);
    if (lane == 0) words[g] = acc;
}

// Erosion, the column pass: the AND of the 2 ey + 1 row-eroded words above and below (those inside the image) says which of the
// wave's 64 pixels keep their depth; the others' depth is cleared in place.
__global__ void __launch_bounds__(BLOCK) rgbd_erode_cols_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam, uint32_t total_words, int ey,
                                                               const unsigned long long *__restrict__ words) {
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * (uint32_t)WAVES + (threadIdx.x >> 6);
    if (g >= total_words) return;
    const RgbdRawCamDev &c = cams[camera_of_word(cams, ncam, g)];
    const uint32_t local = g - c.wfirst, row = local / c.wpr, wi = local - row * c.wpr;
    const uint32_t lo = row > (uint32_t)ey ? row - (uint32_t)ey : 0u, hi = row + (uint32_t)ey < c.height ? row + (uint32_t)ey : c.height - 1u;
    unsigned long long acc = ~0ull;
    for (uint32_t r = lo; r <= hi; r++) acc &= words[(size_t)c.wfirst + (size_t)r * c.wpr + wi];
    const uint32_t u = wi * 64u + (uint32_t)lane;
    if (u < c.width && !((acc >> lane) & 1ull)) c.depth_rw[(size_t)row * c.width + u] = 0;
}

// What the z-splat and the registration both ask of depth pixel p of camera c: is it a candidate (depth after erosion, a colour pixel),
// and then its colour pixel and its depth along the colour camera's axis.  The one evaluation both kernels share, so their bits agree.
__device__ __forceinline__ bool colour_of(const RgbdRawCamDev &c, uint32_t p, unsigned d, int at[2], double &pz) {
    const int v = (int)(p / c.width), u = (int)(p - (uint32_t)v * c.width);
    const double z = rgbd_z(d, c.t.depth_scale);
    double xc, yc;
    rgbd_raw_xy(c.t, c.rays ? c.rays + 2 * (size_t)p : nullptr, u, v, z, xc, yc);
    return rgbd_colour_pixel_depth(c.ct, xc, yc, z, at, pz);
}

// The z-buffer of the colour grids: one lane per depth pixel of the frame.  A candidate's key goes, by atomic minimum, to the cell of
// its own colour pixel: (uc, vc) is in range by rgbd_colour_pixel_depth's test on the doubles, so the cell is one of this camera's
// Wc * Hc words behind zfirst.  The square of the rule is NOT written here -- with (2 splat + 1)^2 atomics per candidate the grab's
// kernels took 3.7 (splat 1) to 8 (splat 2) times the plain grab's, DESIGN 3.19 -- but read by the registration: the minimum over a
// candidate's square of these words is the minimum over the candidates whose squares reach its pixel, the same set.
__global__ void __launch_bounds__(BLOCK) rgbd_zsplat_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam, uint32_t total,
                                                           unsigned long long *__restrict__ zbuf) {
    const uint32_t g = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
    if (g >= total) return;
    const RgbdRawCamDev &c = cams[camera_of(cams, ncam, 0, g)];
    const uint32_t p = g - c.first;
    const unsigned d = c.depth[p];
    if (d == 0u) return;
    int at[2];
    double pz;
    if (!colour_of(c, p, d, at, pz)) return;
    (void)__hip_atomic_fetch_min(zbuf + c.zfirst + (size_t)at[1] * (size_t)c.ct.width + (size_t)at[0], rgbd_depth_key(pz), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
}

// Registration: one lane per depth pixel of the frame.  A pixel with depth takes the colour of the colour pixel its point projects to
// (rgbd_colour_pixel) or, having none, loses its depth; every pixel's registered colour is written, black where there is none.  The
// colour index is in range by rgbd_colour_pixel's test on the doubles; p < the camera's pixel count.  OCCLUSION: Zmin at a candidate's
// colour pixel is the smallest z-buffer word of its square, clipped to the colour image before an index is formed (rgbd_splat_box:
// plain loads, the neighbouring lanes' squares overlap); a candidate that something nearer hides (rgbd_occluded) has no colour either.
template <bool OCCLUSION>
__global__ void __launch_bounds__(BLOCK) rgbd_register_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam, uint32_t total,
                                                             const unsigned long long *__restrict__ zbuf, int splat, double margin) {
    const uint32_t g = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
    if (g >= total) return;
    const RgbdRawCamDev &c = cams[camera_of(cams, ncam, 0, g)];
    const uint32_t p = g - c.first;
    const unsigned d = c.depth[p];
    uint32_t rgb = 0;
    if (d != 0u) {
        int at[2];
        double pz;
        bool has = colour_of(c, p, d, at, pz);
        if constexpr (OCCLUSION) {
            if (has) {
                int lo[2], hi[2];
                rgbd_splat_box(c.ct, at, splat, lo, hi);
                const unsigned long long *__restrict__ plane = zbuf + c.zfirst;
                unsigned long long key_min = RGBD_KEY_EMPTY;
                for (int r = lo[1]; r <= hi[1]; r++) {
                    const unsigned long long *line = plane + (size_t)r * (size_t)c.ct.width;
                    for (int q = lo[0]; q <= hi[0]; q++) {
                        const unsigned long long key = line[q];
                        key_min = key < key_min ? key : key_min;
                    }
                }
                has = !rgbd_occluded(key_min, pz, margin);
            }
        }
        if (has) rgb = load_colour(c.raw_colour, (uint32_t)at[1] * (uint32_t)c.ct.width + (uint32_t)at[0], c.raw_bpp);
        else c.depth_rw[p] = 0;
    }
    uint8_t *out = c.registered + (size_t)p * 3u;
    out[0] = (uint8_t)rgb; out[1] = (uint8_t)(rgb >> 8); out[2] = (uint8_t)(rgb >> 16);
}

// ---- decimation and hole filling (rgbd_decimate.hpp), DESIGN 3.23 ----
//
// Decimation by K.  A workgroup owns a tile of DEC_W x DEC_H pixels of one camera's decimated image, one per lane, and so K * DEC_H
// source rows of K * DEC_W pixels.  A lane does NOT fetch its K * K source pixels itself (K * K two-byte loads, K * 2 bytes apart from
// its neighbour's): the workgroup brings every source row in with 16-byte loads, 1 KB contiguous per wave, and shares them through LDS.
// A source row starts wherever its image's width puts it, so a row's loads start at the 16-byte boundary at or below its first
// pixel and the row keeps that offset (0 .. 7 pixels) in LDS; the vectors are whole in global memory because the host leaves the
// image 16-byte aligned with readable bytes up to the next boundary behind it.  Rows from K * H' and columns from K * W' on belong to
// no block: such rows are not loaded, such columns only as the rest of a vector that nobody reads.
constexpr int DEC_W = 128;
constexpr int DEC_H = BLOCK / DEC_W;

__host__ __device__ __forceinline__ uint32_t decimate_tiles(uint32_t width, uint32_t height) {
    return ((width + (uint32_t)DEC_W - 1u) / (uint32_t)DEC_W) * ((height + (uint32_t)DEC_H - 1u) / (uint32_t)DEC_H);
}

template <int K>
__global__ void __launch_bounds__(BLOCK) rgbd_decimate_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam) {
    constexpr uint32_t SPAN = K * DEC_W;          // source pixels of a full tile's row
    constexpr uint32_t STRIDE = SPAN + 8;         // of a row in LDS, in pixels: the up to 7 pixels in front of the span come with its first vector
    __shared__ uint4 tile4[K * DEC_H * STRIDE / 8];
    const uint16_t *tile = reinterpret_cast<const uint16_t *>(tile4);
    // the camera of this tile and the tile's number in it
    uint32_t t = blockIdx.x;
    int k = 0;
    for (; k < ncam; k++) {
        const uint32_t n = decimate_tiles(cams[k].width, cams[k].height);
        if (t < n) break;
        t -= n;
    }
    if (k == ncam) return;   // (the whole workgroup; the host launches exactly the tiles there are)
    const RgbdRawCamDev &c = cams[k];
    const uint32_t tiles_x = (c.width + (uint32_t)DEC_W - 1u) / (uint32_t)DEC_W;
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t u0 = tx * (uint32_t)DEC_W, v0 = ty * (uint32_t)DEC_H;
    const uint32_t nu = c.width - u0 < (uint32_t)DEC_W ? c.width - u0 : (uint32_t)DEC_W, nv = c.height - v0 < (uint32_t)DEC_H ? c.height - v0 : (uint32_t)DEC_H;
    const uint32_t span = nu * (uint32_t)K, nrows = nv * (uint32_t)K;
    // source row r of the tile: pixels first(r) .. first(r) + span - 1 of the full image, all inside it: (K v0 + r) < K H' <= H and
    // K u0 + span <= K W' <= W
    const auto first = [&](uint32_t r) { return (size_t)((uint32_t)K * v0 + r) * (size_t)c.full_width + (size_t)((uint32_t)K * u0); };
    const uint32_t nvec = (span + 14u) / 8u;      // at most: 7 pixels in front, span, up to the next boundary; <= STRIDE / 8
    const uint4 *__restrict__ full4 = reinterpret_cast<const uint4 *>(c.full_depth);
    for (uint32_t idx = threadIdx.x; idx < nrows * nvec; idx += (uint32_t)BLOCK) {
        const uint32_t r = idx / nvec, i = idx - r * nvec;
        const size_t e0 = first(r), a0 = e0 & ~(size_t)7;
        if (i * 8u < (uint32_t)(e0 - a0) + span) tile4[r * (STRIDE / 8u) + i] = full4[a0 / 8u + i];
    }
    __syncthreads();
    const uint32_t u = threadIdx.x % (uint32_t)DEC_W, v = threadIdx.x / (uint32_t)DEC_W;
    if (u >= nu || v >= nv) return;
    uint16_t block[K * K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const uint32_t r = v * (uint32_t)K + (uint32_t)j;
        const uint16_t *row = tile + r * STRIDE + (uint32_t)(first(r) & (size_t)7) + u * (uint32_t)K;
#pragma unroll
        for (int i = 0; i < K; i++) block[j * K + i] = row[i];
    }
    c.depth_rw[(size_t)(v0 + v) * c.width + u0 + u] = rgbd_block_value<K>(block);
}

// Hole filling from the left (rule 0c, mode 1): out[i] = op(out[i - 1], d[i]) is a scan with an associative operator, so a row is NOT
// walked as the spatial filter's lines are.  One wave per row.  A lane owns 8 neighbouring pixels -- one 16-byte vector, taken at the
// 16-byte boundaries of the image, so the first and the last vector of a row may hold pixels of the rows beside it: those are read as
// 0, the operator's identity, and never written (such a vector is stored pixel by pixel) -- folds them, the wave scans the 64 folds
// with shuffles (6 steps), and every lane runs over its pixels again from what is left of it.  A row longer than 512 pixels takes
// more than one such chunk: `carry`, the last value with depth of the chunks before, goes in front of the next one's scan.
constexpr int FILL_PPL = 8;
constexpr int FILL_CHUNK = 64 * FILL_PPL;

__global__ void __launch_bounds__(BLOCK) rgbd_holefill_left_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam, uint32_t rows) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t row = blockIdx.x * (uint32_t)WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;   // (the whole wave)
    int k = 0;
    while (k + 1 < ncam && row >= cams[k].height) {
        row -= cams[k].height;
        k++;
    }
    const RgbdRawCamDev &c = cams[k];
    const size_t e0 = (size_t)row * c.width, e1 = e0 + c.width;   // the row's pixels in its image
    uint16_t carry = 0;
    for (size_t base = e0 & ~(size_t)7; base < e1; base += (size_t)FILL_CHUNK) {   // (the same trip count in every lane)
        const size_t at = base + (size_t)lane * (size_t)FILL_PPL;   // at + 8 > e0 always
        const bool any = at < e1, whole = at >= e0 && at + (size_t)FILL_PPL <= e1;
        uint16_t v[FILL_PPL];
#pragma unroll
        for (int j = 0; j < FILL_PPL; j++) v[j] = 0;
        if (any) {   // at < e1 <= the image's pixels: the vector ends at or before the 16-byte boundary behind the image
            const uint4 w = *reinterpret_cast<const uint4 *>(c.depth_rw + at);
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < FILL_PPL; j++) {
                const bool mine = at + (size_t)j >= e0 && at + (size_t)j < e1;
                v[j] = mine ? (uint16_t)(words[j >> 1] >> (16 * (j & 1))) : (uint16_t)0;
            }
        }
        uint16_t fold = 0;
#pragma unroll
        for (int j = 0; j < FILL_PPL; j++) fold = rgbd_fill_op(fold, v[j]);
        uint32_t x = fold;   // the inclusive scan of the folds, lane 0 first
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t left = (uint32_t)__shfl_up((int)x, d);
            if (lane >= d) x = rgbd_fill_op((uint16_t)left, (uint16_t)x);
        }
        const uint32_t before = (uint32_t)__shfl_up((int)x, 1u);
        uint16_t run = rgbd_fill_op(carry, lane == 0u ? (uint16_t)0 : (uint16_t)before);
        carry = rgbd_fill_op(carry, (uint16_t)__shfl((int)x, 63));
#pragma unroll
        for (int j = 0; j < FILL_PPL; j++) {
            run = rgbd_fill_op(run, v[j]);
            v[j] = run;
        }
        if (whole) {
            uint4 w;
            w.x = (uint32_t)v[0] | ((uint32_t)v[1] << 16); w.y = (uint32_t)v[2] | ((uint32_t)v[3] << 16);
            w.z = (uint32_t)v[4] | ((uint32_t)v[5] << 16); w.w = (uint32_t)v[6] | ((uint32_t)v[7] << 16);
            *reinterpret_cast<uint4 *>(c.depth_rw + at) = w;
        } else if (any) {
#pragma unroll
            for (int j = 0; j < FILL_PPL; j++)
                if (at + (size_t)j >= e0 && at + (size_t)j < e1) c.depth_rw[at + (size_t)j] = v[j];
        }
    }
}

// Hole filling from around (rule 0c, modes 2 and 3): one lane per depth pixel of the frame.  The rule reads the stage's input, so
// the first launch writes every pixel's new value to a plane of its own (scratch, in pixel-number order) and the second copies the
// plane over the images.  Only a pixel without depth looks at its neighbours, each inside the image before an index is formed.
template <bool BACK>
__global__ void __launch_bounds__(BLOCK) rgbd_holefill_around_kernel(const RgbdRawCamDev *__restrict__ cams, int ncam, uint32_t total, int mode,
                                                                    uint16_t *__restrict__ scratch) {
    const uint32_t g = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
    if (g >= total) return;
    const RgbdRawCamDev &c = cams[camera_of(cams, ncam, 0, g)];
    const uint32_t p = g - c.first;
    if constexpr (BACK) {
        c.depth_rw[p] = scratch[g];
    } else {
        const uint16_t d = c.depth[p];
        if (d != 0) {
            scratch[g] = d;
            return;
        }
        const int width = (int)c.width, height = (int)c.height;
        const int v = (int)(p / c.width), u = (int)(p - (uint32_t)v * c.width);
        uint16_t n[9];
#pragma unroll
        for (int dv = -1; dv <= 1; dv++) {
#pragma unroll
            for (int du = -1; du <= 1; du++) {
                const int y = v + dv, x = u + du;
                const bool inside = y >= 0 && y < height && x >= 0 && x < width;
                n[(dv + 1) * 3 + du + 1] = inside ? c.depth[(size_t)y * c.width + (size_t)x] : (uint16_t)0;
            }
        }
        scratch[g] = rgbd_fill_pick(mode, n);
    }
}

template <int K>
void decimate_launch(const RgbdRawCamDev *cams, int ncam, uint32_t tiles, hipStream_t s) {
    CW_LAUNCH("rgbd_decimate", rgbd_decimate_kernel<K>, dim3(tiles), dim3(BLOCK), 0, s, cams, ncam);
}

}  // namespace

void rgbd_count(const RgbdCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, uint32_t *counts, uint32_t *ticket,
                unsigned long long *total_host, uint32_t tag, hipStream_t s) {
    count_launch(cams, ncam, total_pixels, f, counts, ticket, total_host, tag, s);
}

void rgbd_scatter(const RgbdCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, const uint32_t *offsets, const DeviceSoA &dst,
                  hipStream_t s) {
    scatter_launch(cams, ncam, total_pixels, f, offsets, dst, s);
}

void rgbd_count(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, uint32_t *counts, uint32_t *ticket,
                unsigned long long *total_host, uint32_t tag, hipStream_t s) {
    count_launch(cams, ncam, total_pixels, f, counts, ticket, total_host, tag, s);
}

void rgbd_scatter(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, const RgbdFilterTerms &f, const uint32_t *offsets, const DeviceSoA &dst,
                  hipStream_t s) {
    scatter_launch(cams, ncam, total_pixels, f, offsets, dst, s);
}

uint32_t rgbd_line_groups(uint32_t lines) { return line_groups(lines); }

void rgbd_spatial(const RgbdRawCamDev *cams, int ncam, uint32_t row_groups, uint32_t col_groups, int magnitude, const RgbdSmoothTerms &t, hipStream_t s) {
    for (int it = 0; it < magnitude; it++) {
        CW_LAUNCH("rgbd_spatial_rows", rgbd_spatial_kernel<true>, dim3(row_groups), dim3(64), 0, s, cams, ncam, t);
        CW_LAUNCH("rgbd_spatial_cols", rgbd_spatial_kernel<false>, dim3(col_groups), dim3(64), 0, s, cams, ncam, t);
    }
}

void rgbd_temporal(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, const RgbdSmoothTerms &t, int persistency, double *value, uint8_t *history,
                   hipStream_t s) {
    CW_LAUNCH("rgbd_temporal", rgbd_temporal_kernel, dim3((unsigned)(((size_t)total_pixels + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, cams, ncam,
              total_pixels, t, persistency, value, history);
}

void rgbd_erode(const RgbdRawCamDev *cams, int ncam, uint32_t total_words, int ex, int ey, unsigned long long *words, hipStream_t s) {
    const dim3 grid((unsigned)(((size_t)total_words + WAVES - 1) / WAVES));
    CW_LAUNCH("rgbd_erode_rows", rgbd_erode_rows_kernel, grid, dim3(BLOCK), 0, s, cams, ncam, total_words, ex, words);
    CW_LAUNCH("rgbd_erode_cols", rgbd_erode_cols_kernel, grid, dim3(BLOCK), 0, s, cams, ncam, total_words, ey, (const unsigned long long *)words);
}

void rgbd_register(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, hipStream_t s) {
    CW_LAUNCH("rgbd_register", rgbd_register_kernel<false>, dim3((unsigned)(((size_t)total_pixels + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, cams, ncam,
              total_pixels, (const unsigned long long *)nullptr, 0, 0.0);
}

void rgbd_zsplat(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, unsigned long long *zbuf, hipStream_t s) {
    CW_LAUNCH("rgbd_zsplat", rgbd_zsplat_kernel, dim3((unsigned)(((size_t)total_pixels + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, cams, ncam,
              total_pixels, zbuf);
}

void rgbd_register_occluded(const RgbdRawCamDev *cams, int ncam, uint32_t total_pixels, const unsigned long long *zbuf, int splat, double margin,
                            hipStream_t s) {
    CW_LAUNCH("rgbd_register_occluded", rgbd_register_kernel<true>, dim3((unsigned)(((size_t)total_pixels + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, cams,
              ncam, total_pixels, zbuf, splat, margin);
}

uint32_t rgbd_decimate_tiles(uint32_t width, uint32_t height) { return decimate_tiles(width, height); }

void rgbd_decimate(const RgbdRawCamDev *cams, int ncam, int k, uint32_t tiles, hipStream_t s) {
    switch (k) {
        case 2: decimate_launch<2>(cams, ncam, tiles, s); break;
        case 3: decimate_launch<3>(cams, ncam, tiles, s); break;
        case 4: decimate_launch<4>(cams, ncam, tiles, s); break;
        case 5: decimate_launch<5>(cams, ncam, tiles, s); break;
        case 6: decimate_launch<6>(cams, ncam, tiles, s); break;
        case 7: decimate_launch<7>(cams, ncam, tiles, s); break;
        case 8: decimate_launch<8>(cams, ncam, tiles, s); break;
        default: break;   // (1: nothing to do; the host has refused everything else)
    }
}

void rgbd_holefill(const RgbdRawCamDev *cams, int ncam, int mode, uint32_t rows, uint32_t total_pixels, uint16_t *scratch, hipStream_t s) {
    if (mode == 1) {
        CW_LAUNCH("rgbd_holefill_left", rgbd_holefill_left_kernel, dim3((unsigned)(((size_t)rows + WAVES - 1) / WAVES)), dim3(BLOCK), 0, s, cams, ncam, rows);
    } else if (mode == 2 || mode == 3) {
        const dim3 grid((unsigned)(((size_t)total_pixels + BLOCK - 1) / BLOCK));
        CW_LAUNCH("rgbd_holefill_around", rgbd_holefill_around_kernel<false>, grid, dim3(BLOCK), 0, s, cams, ncam, total_pixels, mode, scratch);
        CW_LAUNCH("rgbd_holefill_around", rgbd_holefill_around_kernel<true>, grid, dim3(BLOCK), 0, s, cams, ncam, total_pixels, mode, scratch);
    }
}

}  // namespace k
}  // namespace cwipc_amd
