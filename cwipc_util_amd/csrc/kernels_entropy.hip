// kernels_entropy.hip -- gfx950 kernels of the entropy-coded packet form (RULE E: hip_ext.h; the arithmetic: entropy_terms.hpp).
//
// Encode, on the body that codec_emit left on the device:  histograms per stream (LDS, then integer atomics: order-free) -> f[] per
// stream (one wave per stream: entropy_normalise's steps with wave-wide maxima) -> the block encoder, one wave per block of 4096 symbols:
// 64 states in registers, f and cum in LDS, a symbol per lane per round, rounds from the last to the first -> the plan (one wave:
// block offsets, payload sizes, the mode of every stream, the directory, the total) -> the gather into one contiguous buffer.
// The words of a block are written ONCE, into the block's slot of 4096 words, from its end backwards: the encoder emits in the
// reverse of the decoder's order, so what it has emitted always sits at the end of the slot in decoder order and the gather copies
// one contiguous run.  (A size pass followed by a write pass would run the divisions of every symbol twice to save 8 KiB per block.)
// The rank of an emitting lane within its round is a ballot and a count of the lanes above it.
//
// Decode.  One wave per block: the slot search over cum in LDS (8 steps over 256 entries; a 4096-entry table would cost a wave more
// to fill than its 64 rounds save), the words of a round taken in lane order (ballot, count of the lanes below), the block-local scan
// of the colour differences, then the three channel planes repacked into RULE C's colour plane (32 leaves are 3 cb whole words: plain
// stores), then the check.  For ANY bytes every read of a block goes through entropy_word() (bounded by the block's size), every
// slot lookup through entropy_find() (0..255) and every store is bounded by the header's counts.
#include "internal.hpp"
#include "block_scan.hpp"
#include "entropy_terms.hpp"

namespace cwipc_amd {
namespace k {

static constexpr int EB = 256;   // lanes of the histogram and gather workgroups

__device__ __forceinline__ int stream_of_block(const EntropyStreams &st, uint32_t block) {
    int s = 0;
    for (int i = 1; i < st.nstreams; i++)
        if (block >= st.first_block[i]) s = i;
    return s;
}

// cum[] from f[] in LDS by one wave: four entries per lane
__device__ __forceinline__ void wave_cumulate(const uint16_t *f, uint16_t *cum, int lane) {
    const uint32_t a0 = f[4 * lane], a1 = f[4 * lane + 1], a2 = f[4 * lane + 2], a3 = f[4 * lane + 3];
    const uint32_t t = a0 + a1 + a2 + a3;
    uint32_t inc = t;
    for (int off = 1; off < 64; off <<= 1) {   // (kept: with wave_inclusive_scan the encode kernel measured 2 % slower)
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    const uint32_t at = inc - t;
    cum[4 * lane] = (uint16_t)at;
    cum[4 * lane + 1] = (uint16_t)(at + a0);
    cum[4 * lane + 2] = (uint16_t)(at + a0 + a1);
    cum[4 * lane + 3] = (uint16_t)(at + a0 + a1 + a2);
}

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t colour_value(const uint32_t *__restrict__ colours, uint64_t colour_words, int cb, uint32_t leaf, uint32_t channel) {
    const uint64_t bit = ((uint64_t)leaf * 3u + channel) * (uint64_t)cb;
    const uint64_t word = bit >> 5;
    const uint32_t off = (uint32_t)(bit & 31u);
    uint32_t v = word < colour_words ? colours[word] >> off : 0u;
    if (off + (uint32_t)cb > 32u && word + 1 < colour_words) v |= colours[word + 1] << (32u - off);
    return v & ((1u << cb) - 1u);
}

// the plain value j of stream s (j < symbols)
__device__ __forceinline__ uint32_t stream_value(const EntropyEncode &e, int s, uint32_t j) {
    const uint32_t kind = e.st.kind[s];
    if (kind == ENTROPY_OCCUPANCY) return e.occupancy[(size_t)e.st.plane_offset[s] + j];
    if (kind == ENTROPY_TILE) return e.tiles[j];
    if (kind == ENTROPY_BYTES || kind == ENTROPY_BITS) return e.planes[(size_t)e.st.plane_offset[s] + j];
    return colour_value(e.colours, e.colour_words, e.st.colour_bits, j, e.st.which[s]);
}

// the symbol that is coded: for a colour the difference to the leaf before, the first of a block as it is
__device__ __forceinline__ uint32_t stream_symbol(const EntropyEncode &e, int s, uint32_t j) {
    const uint32_t v = stream_value(e, s, j);
    if (e.st.kind[s] != ENTROPY_COLOUR || (j % ENTROPY_BLOCK) == 0u) return v;
    return (v - stream_value(e, s, j - 1u)) & ((1u << e.st.colour_bits) - 1u);
}

__global__ void __launch_bounds__(EB) entropy_hist_kernel(EntropyEncode e) {
    __shared__ uint32_t h[256];
    const int s = stream_of_block(e.st, blockIdx.x);
    const uint32_t symbols = e.st.symbols[s];
    if (symbols < ENTROPY_BLOCK) return;   // (such a stream stays raw)
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t first = (blockIdx.x - e.st.first_block[s]) * ENTROPY_BLOCK;
    for (uint32_t i = threadIdx.x; i < ENTROPY_BLOCK; i += EB) {
        const uint32_t j = first + i;
        if (j < symbols) atomicAdd(&h[stream_symbol(e, s, j) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&e.hist[(size_t)s * 256 + threadIdx.x], h[threadIdx.x]);
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// entropy_normalise() by one wave per stream, symbols 4 l .. 4 l + 3 in lane l.  "The largest, the lowest symbol on ties" is the
// maximum of value << 8 | (255 - symbol); the serial loop's decrements are taken one by one, each a wave-wide maximum (at most 255
// of them), so the result is the host function's for every count vector -- the tests hold the two to each other through the bytes.
__global__ void __launch_bounds__(64) entropy_normalise_kernel(EntropyEncode e) {
    const int s = blockIdx.x, lane = threadIdx.x;
    if (e.st.symbols[s] < ENTROPY_BLOCK) return;
    uint32_t c[4], f[4];
    unsigned long long total = 0, best = 0;
    for (int k = 0; k < 4; k++) {
        c[k] = e.hist[(size_t)s * 256 + 4 * lane + k];
        total += c[k];
        const unsigned long long key = ((unsigned long long)c[k] << 8) | (unsigned long long)(255 - (4 * lane + k));
        best = key > best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
    best = wave_max(best);
    if (total == 0ull) return;
    uint32_t sum = 0;
    for (int k = 0; k < 4; k++) {
        f[k] = 0;
        if (c[k]) {
            f[k] = (uint32_t)(((unsigned long long)c[k] * ENTROPY_M) / total);
            if (f[k] < 1u) f[k] = 1u;
        }
        sum += f[k];
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    int d = (int)ENTROPY_M - (int)sum;
    if (d > 0) {
        const int top = 255 - (int)(best & 255ull);
        for (int k = 0; k < 4; k++)
            if (4 * lane + k == top) f[k] += (uint32_t)d;
    }
    for (; d < 0; d++) {
        unsigned long long key = 0;
        for (int k = 0; k < 4; k++) {
            const unsigned long long mine = ((unsigned long long)f[k] << 8) | (unsigned long long)(255 - (4 * lane + k));
            key = mine > key ? mine : key;
        }
        const int top = 255 - (int)(wave_max(key) & 255ull);
        for (int k = 0; k < 4; k++)
            if (4 * lane + k == top) f[k] -= 1u;
    }
    for (int k = 0; k < 4; k++) e.freq[(size_t)s * 256 + 4 * lane + k] = (uint16_t)f[k];
}

__global__ void __launch_bounds__(64) entropy_block_encode_kernel(EntropyEncode e) {
    __shared__ uint16_t f[256], cum[256];
    const uint32_t block = blockIdx.x;
    const int s = stream_of_block(e.st, block), lane = threadIdx.x;
    const uint32_t symbols = e.st.symbols[s];
    if (symbols < ENTROPY_BLOCK) {
        if (lane == 0) { e.block_words[block] = 0; e.block_bytes[block] = 0; }
        return;
    }
    for (int i = lane; i < 256; i += 64) f[i] = e.freq[(size_t)s * 256 + i];
    __syncthreads();
    wave_cumulate(f, cum, lane);
    __syncthreads();
    const uint32_t local = block - e.st.first_block[s], first = local * ENTROPY_BLOCK;
    const uint32_t m = entropy_block_symbols(symbols, local);
    uint8_t *slot = e.slots + (size_t)block * ENTROPY_SLOT_BYTES;
    uint16_t *words = reinterpret_cast<uint16_t *>(slot + ENTROPY_STATES_BYTES);
    uint32_t x = ENTROPY_LOW, emitted = 0;
    for (uint32_t r = (m + 63u) / 64u; r-- > 0;) {
        const uint32_t j = 64u * r + (uint32_t)lane;
        bool emit = false;
        uint16_t w = 0;
        if (j < m) {
            const uint32_t sym = stream_symbol(e, s, first + j) & 255u;
            const uint32_t fs = f[sym];
            if (fs) emit = entropy_put(x, fs, cum[sym], w);   // (fs > 0: the symbol was counted)
        }
        const unsigned long long b = __ballot(emit);
        if (emit) {
            const uint32_t above = (uint32_t)__popcll((b >> lane) >> 1);   // lanes descend within a round
            const uint32_t at = emitted + above;
            if (at < ENTROPY_BLOCK) words[ENTROPY_BLOCK - 1u - at] = w;
        }
        emitted += (uint32_t)__popcll(b);
    }
    reinterpret_cast<uint32_t *>(slot)[lane] = x;
    if (lane == 0) {
        e.block_words[block] = emitted;
        e.block_bytes[block] = entropy_block_bytes(emitted);
    }
}

// one wave: per stream the offsets of its blocks, the size of its coded payload, its mode; the directory; the report
__global__ void __launch_bounds__(64) entropy_plan_kernel(EntropyEncode e) {
    const int lane = threadIdx.x;
    int S = e.st.nstreams;
    if (S > 0 && e.st.kind[S - 1] == ENTROPY_TILE && (e.tile_stats[0] & e.tile_stats[1]) == 0u) S--;   // uniform tiles: no tile plane
    uint64_t at = 4u + 8u * (uint64_t)S;
    for (int s = 0; s < S; s++) {
        const uint32_t nb = entropy_block_count(e.st.symbols[s]), first = e.st.first_block[s];
        uint32_t running = 0;
        if (e.st.symbols[s] >= ENTROPY_BLOCK) {
            for (uint32_t base = 0; base < nb; base += 64u) {
                const uint32_t i = base + (uint32_t)lane;
                const uint32_t v = i < nb ? e.block_bytes[first + i] : 0u;
                const uint32_t inc = wave_inclusive_scan(v);
                if (i < nb) e.block_offset[first + i] = running + inc - v;
                running += __shfl(inc, 63, 64);
            }
        }
        const uint64_t coded = (uint64_t)ENTROPY_TABLE_BYTES + 4u * (uint64_t)nb + running;
        const uint32_t mode = e.st.symbols[s] >= ENTROPY_BLOCK && coded < (uint64_t)e.st.raw_padded[s] ? 1u : 0u;
        const uint32_t bytes = mode ? (uint32_t)coded : e.st.raw_padded[s];
        if (lane == 0) {
            e.plan[3 * s] = mode;
            e.plan[3 * s + 1] = (uint32_t)at;
            e.plan[3 * s + 2] = bytes;
            if (12u + 8u * (uint64_t)s <= e.out_capacity) {
                uint32_t *entry = reinterpret_cast<uint32_t *>(e.out + 4u + 8u * (size_t)s);
                entry[0] = mode;
                entry[1] = bytes;
            }
        }
        at += bytes;
    }
    if (lane == 0) {
        for (int s = S; s < e.st.nstreams; s++) { e.plan[3 * s] = 2u; e.plan[3 * s + 1] = 0; e.plan[3 * s + 2] = 0; }   // 2: not in the packet
        if (e.out_capacity >= 4u) *reinterpret_cast<uint32_t *>(e.out) = (uint32_t)S;
        e.report[0] = (uint32_t)(at <= e.out_capacity ? at : 0u);
        e.report[1] = (uint32_t)S;
        e.report[2] = e.tile_stats[0];
        e.report[3] = e.tile_stats[1];
    }
}

__global__ void __launch_bounds__(EB) entropy_gather_kernel(EntropyEncode e) {
    const uint32_t block = blockIdx.x;
    const int s = stream_of_block(e.st, block);
    const uint32_t mode = e.plan[3 * s], payload = e.plan[3 * s + 1], bytes = e.plan[3 * s + 2];
    if (mode > 1u || (uint64_t)payload + bytes > e.out_capacity) return;
    const uint32_t symbols = e.st.symbols[s], local = block - e.st.first_block[s];
    uint8_t *dst = e.out + payload;
    if (mode == 1u) {
        const uint32_t nb = entropy_block_count(symbols);
        if (local == 0) reinterpret_cast<uint16_t *>(dst)[threadIdx.x] = e.freq[(size_t)s * 256 + threadIdx.x];
        const uint32_t size = e.block_bytes[block], count = e.block_words[block];
        const uint64_t at = (uint64_t)ENTROPY_TABLE_BYTES + 4u * (uint64_t)nb + e.block_offset[block];
        if (at + size > bytes || count > ENTROPY_BLOCK) return;
        if (threadIdx.x == 0) reinterpret_cast<uint32_t *>(dst + ENTROPY_TABLE_BYTES)[local] = size;
        const uint8_t *slot = e.slots + (size_t)block * ENTROPY_SLOT_BYTES;
        if (threadIdx.x < 64) reinterpret_cast<uint32_t *>(dst + at)[threadIdx.x] = reinterpret_cast<const uint32_t *>(slot)[threadIdx.x];
        const uint16_t *from = reinterpret_cast<const uint16_t *>(slot + ENTROPY_STATES_BYTES) + (ENTROPY_BLOCK - count);
        uint16_t *to = reinterpret_cast<uint16_t *>(dst + at + ENTROPY_STATES_BYTES);
        for (uint32_t i = threadIdx.x; i < count; i += EB) to[i] = from[i];   // (the padding word is the zero the buffer was filled with)
        return;
    }
    const uint32_t first = local * ENTROPY_BLOCK;
    if (!entropy_kind_packed(e.st.kind[s])) {
        for (uint32_t i = threadIdx.x; i < ENTROPY_BLOCK; i += EB) {
            const uint32_t j = first + i;
            if (j < symbols && j < bytes) dst[j] = (uint8_t)stream_value(e, s, j);
        }
        return;
    }
    // 32 values of cb bits are cb whole words
    const uint32_t cb = (uint32_t)e.st.colour_bits;
    if (threadIdx.x >= ENTROPY_BLOCK / 32u) return;
    const uint32_t j0 = first + 32u * threadIdx.x;
    if (j0 >= symbols) return;
    uint32_t *to = reinterpret_cast<uint32_t *>(dst);
    uint64_t word = (uint64_t)(j0 / 32u) * cb, acc = 0;
    uint32_t have = 0;
    for (uint32_t i = 0; i < 32u; i++) {
        const uint32_t j = j0 + i;
        acc |= (uint64_t)(j < symbols ? stream_value(e, s, j) : 0u) << have;
        have += cb;
        if (have >= 32u) {
            if (4u * word + 4u <= bytes) to[word] = (uint32_t)acc;
            word++;
            acc >>= 32;
            have -= 32u;
        }
    }
}

void entropy_encode(const EntropyEncode &e, hipStream_t s) {
    if (!e.st.nstreams || !e.st.total_blocks) return;
    CW_LAUNCH("entropy_hist", entropy_hist_kernel, dim3(e.st.total_blocks), dim3(EB), 0, s, e);
    CW_LAUNCH("entropy_normalise", entropy_normalise_kernel, dim3((unsigned)e.st.nstreams), dim3(64), 0, s, e);
    CW_LAUNCH("entropy_block_encode", entropy_block_encode_kernel, dim3(e.st.total_blocks), dim3(64), 0, s, e);
    CW_LAUNCH("entropy_plan", entropy_plan_kernel, dim3(1), dim3(64), 0, s, e);
    CW_LAUNCH("entropy_gather", entropy_gather_kernel, dim3(e.st.total_blocks), dim3(EB), 0, s, e);
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) entropy_block_decode_kernel(EntropyDecode d) {
    __shared__ uint16_t f[256], cum[256];
    const uint32_t block = blockIdx.x;
    const int s = stream_of_block(d.st, block), lane = threadIdx.x;
    const uint32_t symbols = d.st.symbols[s], kind = d.st.kind[s], local = block - d.st.first_block[s];
    const uint32_t first = local * ENTROPY_BLOCK, m = entropy_block_symbols(symbols, local);
    const uint32_t cb = (uint32_t)d.st.colour_bits, mask = (1u << cb) - 1u;
    const uint8_t *payload = d.in + d.payload_offset[s];
    uint8_t *plain = kind == ENTROPY_OCCUPANCY ? d.occupancy + d.st.plane_offset[s]
                     : kind == ENTROPY_TILE    ? d.tiles
                     : kind == ENTROPY_COLOUR  ? d.channels + (size_t)d.st.which[s] * d.st.nleaves
                                               : d.planes + d.st.plane_offset[s];
    if (d.mode[s] == 0u) {
        // raw: the bytes as they are (the host has tested a raw occupancy stream), a colour's cb-bit values unpacked
        for (uint32_t i = lane; i < m; i += 64u) {
            const uint32_t j = first + i;
            plain[j] = entropy_kind_packed(kind) ? (uint8_t)entropy_bits_at(payload, d.payload_bytes[s], (uint64_t)j * cb, (int)cb) : payload[j];
        }
        return;
    }
    for (int i = lane; i < 256; i += 64) f[i] = (uint16_t)(payload[2 * i] | (payload[2 * i + 1] << 8));
    __syncthreads();
    wave_cumulate(f, cum, lane);
    __syncthreads();
    const uint32_t at = d.block_at[2 * block], bytes = d.block_at[2 * block + 1];   // the host has held them to the payload
    const uint8_t *data = d.in + at, *words = data + ENTROPY_STATES_BYTES;
    const uint32_t count = (bytes - ENTROPY_STATES_BYTES) / 2u;
    uint32_t x = (uint32_t)data[4 * lane] | ((uint32_t)data[4 * lane + 1] << 8) | ((uint32_t)data[4 * lane + 2] << 16) | ((uint32_t)data[4 * lane + 3] << 24);
    uint32_t bad = x < ENTROPY_LOW ? 1u : 0u, cursor = 0, carry = 0, zero = 0, children = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < (m + 63u) / 64u; r++) {
        const uint32_t j = 64u * r + (uint32_t)lane;
        const bool live = j < m;
        uint32_t sym = 0;
        if (live) sym = entropy_get(x, f, cum);
        const bool need = live && x < ENTROPY_LOW;
        const unsigned long long b = __ballot(need);
        if (need) x = (x << 16) | entropy_word(words, count, cursor + (uint32_t)__popcll(b & below), bad);
        cursor += (uint32_t)__popcll(b);
        if (kind == ENTROPY_COLOUR) {
            const uint32_t inc = wave_inclusive_scan(sym);   // the differences add up within the block, mod 2^cb
            sym = (carry + inc) & mask;
            carry = __shfl(sym, 63, 64);
        } else if (kind == ENTROPY_OCCUPANCY && live) {
            if (sym == 0u) zero = 1u;
            children += (uint32_t)__popc(sym);
        }
        if (live) plain[first + j] = (uint8_t)sym;
    }
    if (x != ENTROPY_LOW) bad = 1u;
    if (lane == 0 && !entropy_cursor_at_end(words, count, cursor)) bad = 1u;
    const uint32_t status = (__any(bad != 0u) ? 1u : 0u) | (__any(zero != 0u) ? 2u : 0u);
    if (kind == ENTROPY_OCCUPANCY) {
        wave_reduce_sum(children);
        if (lane == 0) atomicAdd(&d.flags[1 + s], children);
    }
    if (lane == 0 && status) atomicOr(&d.flags[0], status);
}

// 32 leaves -> 3 cb words of RULE C's colour plane
__global__ void __launch_bounds__(EB) entropy_repack_kernel(EntropyDecode d) {
    const uint64_t group = (uint64_t)blockIdx.x * EB + threadIdx.x;
    const uint64_t j0 = group * 32u;
    const uint32_t n = d.st.nleaves, cb = (uint32_t)d.st.colour_bits;
    if (j0 >= n) return;
    uint64_t word = group * 3u * cb, acc = 0;
    uint32_t have = 0;
    for (uint32_t i = 0; i < 32u; i++) {
        const uint64_t j = j0 + i;
        for (uint32_t ch = 0; ch < 3u; ch++) {
            acc |= (uint64_t)(j < n ? d.channels[(size_t)ch * n + j] : 0u) << have;
            have += cb;
            if (have >= 32u) {
                if (word < d.colour_words) d.colours[word] = (uint32_t)acc;
                word++;
                acc >>= 32;
                have -= 32u;
            }
        }
    }
}

__global__ void __launch_bounds__(64) entropy_check_kernel(EntropyDecode d, unsigned long long *__restrict__ status_host, uint32_t tag) {
    if (threadIdx.x != 0) return;
    uint32_t status = d.flags[0];
    for (int s = 0; s < d.st.nstreams; s++)
        if (d.st.kind[s] == ENTROPY_OCCUPANCY && d.mode[s] == 1u && d.flags[1 + s] != d.children[s]) status |= 4u;
    __hip_atomic_store(status_host, ((unsigned long long)tag << 32) | status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

void entropy_decode(const EntropyDecode &d, unsigned long long *status_host, uint32_t tag, hipStream_t s) {
    if (d.st.total_blocks) {
        CW_LAUNCH("entropy_block_decode", entropy_block_decode_kernel, dim3(d.st.total_blocks), dim3(64), 0, s, d);
        if (d.colours)
            CW_LAUNCH("entropy_repack", entropy_repack_kernel, dim3((unsigned)(((size_t)d.st.nleaves + 32u * EB - 1) / (32u * EB))), dim3(EB), 0, s, d);
    }
    CW_LAUNCH("entropy_check", entropy_check_kernel, dim3(1), dim3(64), 0, s, d, status_host, tag);
}

}  // namespace k
}  // namespace cwipc_amd
