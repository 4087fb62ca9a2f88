// kernels_kde.hip -- 1-D Gaussian kernel density estimate on gfx950.
//
// Reference: scipy.stats.gaussian_kde(samples).evaluate(at) as the registration analyzer calls it
// (python/cwipc/registration/analyze.py:171-179), for one dimension and a bandwidth h the caller has worked out:
//   density[j] = sum_i exp(-0.5 * z * z) / (n * h * sqrt(2 pi)),   z = (at[j] - samples[i]) / h      (f64 throughout)
// (z is formed as (at[j] - samples[i]) * (1 / h): one rounding more than the division, 1e-16 of z, inside what the argument of
// exp carries anyway.)
//
// The sum is taken in two levels, in an order that depends on n alone:
//   * the samples are cut into chunks of KDE_CHUNK << s samples, s the smallest shift that leaves at most KDE_MAX_CHUNKS chunks
//     (s = 0 up to 2^20 samples);
//   * one wave per (chunk, 64 evaluation points): the chunk's samples pass through LDS in blocks of KDE_STAGE, every lane keeps one
//     evaluation point and reads each sample as a broadcast; a lane adds sample i of the chunk to accumulator i mod 4 and
//     closes with (a0 + a1) + (a2 + a3) -- four independent chains of exp and add instead of one;
//   * a second kernel adds the chunks' sums per evaluation point, chunk c to accumulator c mod 4, closed the same way, and divides.
// No atomics, no dependence on the launch shape: the same arrays give the same bits on every call.
#include "internal.hpp"

#include <cmath>

namespace cwipc_amd {

namespace {

constexpr int KDE_WAVE = 64;           // evaluation points per workgroup: one wave
constexpr size_t KDE_CHUNK = 1024;     // samples per chunk before the shift
constexpr size_t KDE_MAX_CHUNKS = 1024;
constexpr int KDE_STAGE = 1024;        // samples in LDS at a time (8 KB)

__global__ void __launch_bounds__(KDE_WAVE) kde_partial_kernel(const double *__restrict__ samples, size_t n, size_t chunk, double inv_h,
                                                              const double *__restrict__ at, size_t m, double *__restrict__ partial) {
    __shared__ double stage[KDE_STAGE];
    const size_t j = (size_t)blockIdx.y * KDE_WAVE + threadIdx.x;
    const double x = j < m ? at[j] : 0.0;
    const size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t base = lo; base < hi; base += KDE_STAGE) {   // (chunk is a multiple of KDE_STAGE, and of 4: sample i of the chunk is slot i mod 4)
        const int cnt = (int)(hi - base < (size_t)KDE_STAGE ? hi - base : (size_t)KDE_STAGE);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += KDE_WAVE) stage[i] = samples[base + i];
        __syncthreads();
        int i = 0;
        for (; i + 4 <= cnt; i += 4) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double z = (x - stage[i + u]) * inv_h;
                acc[u] += exp(-0.5 * z * z);
            }
        }
        for (int u = 0; i + u < cnt; u++) {   // (the last block of the last chunk only)
            const double z = (x - stage[i + u]) * inv_h;
            acc[u] += exp(-0.5 * z * z);
        }
    }
    if (j < m) partial[(size_t)blockIdx.x * m + j] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ void __launch_bounds__(256) kde_final_kernel(const double *__restrict__ partial, size_t nchunks, size_t m, double denom, double *__restrict__ density) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    size_t c = 0;
    for (; c + 4 <= nchunks; c += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) acc[u] += partial[(c + u) * m + j];
    }
    for (int u = 0; c + u < nchunks; u++) acc[u] += partial[(c + u) * m + j];
    density[j] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) / denom;
}

}  // namespace

bool gaussian_kde(const double *dev_samples, size_t n, double h, const double *dev_at, size_t m, double *dev_density) {
    ThreadCtx &c = tctx();
    if (!c.ensure()) return false;
    if (m == 0) return true;
    if (n == 0 || !(h > 0.0) || !std::isfinite(h)) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_gaussian_kde", "needs at least one sample and a positive, finite bandwidth");
        return false;
    }
    size_t chunk = KDE_CHUNK;
    while ((n + chunk - 1) / chunk > KDE_MAX_CHUNKS) chunk <<= 1;
    const size_t nchunks = (n + chunk - 1) / chunk, mtiles = (m + KDE_WAVE - 1) / KDE_WAVE;
    if (mtiles > 65535) {
        cwipc_log(CWIPC_LOG_LEVEL_ERROR, "cwipc_hip_gaussian_kde", "too many evaluation points (4 million at most)");
        return false;
    }
    double *partial = (double *)pool_alloc(nchunks * m * sizeof(double));
    if (!partial) return false;
    const double denom = (double)n * h * sqrt(2.0 * M_PI);
    CW_LAUNCH("kde_partial", kde_partial_kernel, dim3((unsigned)nchunks, (unsigned)mtiles), dim3(KDE_WAVE), 0, c.stream, dev_samples, n, chunk, 1.0 / h, dev_at, m,
              partial);
    CW_LAUNCH("kde_final", kde_final_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c.stream, partial, nchunks, m, denom, dev_density);
    c.free_later(partial);
    return hipGetLastError() == hipSuccess;
}

}  // namespace cwipc_amd
