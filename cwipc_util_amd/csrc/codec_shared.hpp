// codec_shared.hpp -- what the octree codec's encoder (codec_encode.cpp), decoder (codec_decode.cpp) and host entry points
// (codec_host.cpp) share on the host: the holders that give device blocks and a coded packet's upload back on every exit, and RULE P's
// reference on the device.  (The staging arithmetic: codec_stage.hpp, through internal.hpp; the C boundary's guards: c_boundary.hpp.)
#pragma once

#include "internal.hpp"   // (with codec_stage.hpp and, through it, the terms headers of RULE C, E, P and T)
#include "c_boundary.hpp"   // (ErrorbufScope, guarded())
#include "lod_terms.hpp"

#include <deque>

namespace cwipc_amd {

inline size_t round256(size_t n) { return stage_round256(n); }

// an event has come (wait: wait for it)
inline bool event_done(hipEvent_t ev, bool wait) {
    if (wait) return hipEventSynchronize(ev) == hipSuccess;
    const hipError_t e = hipEventQuery(ev);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
}

// the far end of an encoder's or a decoder's queue: closed by the caller, at its end once the queue has been emptied
template <typename T>
bool queue_eof(T *q) {
    if (q == nullptr) return true;
    std::lock_guard<std::mutex> l(q->lock);
    return q->closed && q->queue.empty();
}
template <typename T>
void queue_close(T *q) {
    if (q == nullptr) return;
    std::lock_guard<std::mutex> l(q->lock);
    q->closed = true;
}

// The device blocks of one call.  They go back by hand while nothing that reads them is in flight, and through the calling
// thread's free_later once kernels have been queued (a block handed to free_later returns to the pool in the thread's next wait).
struct DeviceBlocks {
    void *held[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    bool queued = false;   // kernels that read them are in flight on the calling thread's stream
    uint8_t *alloc(size_t bytes) {
        void *p = n < 6 ? pool_alloc(bytes) : nullptr;
        if (p) held[n++] = p;
        return (uint8_t *)p;
    }
    void release() {
        for (int i = 0; i < n; i++)
            if (queued) tctx().free_later(held[i]); else pool_free(held[i]);
        n = 0;
    }
    ~DeviceBlocks() { release(); }
};

// A coded packet (RULE E's container: "cwae", "cwat", a "cwap" delta) on its way to the device: the page-locked staging buffer with
// the bytes from the directory on and the block table behind them, the device block they are copied to (`extra` bytes of the
// caller's behind the upload), and the giving back of both on every exit.
struct CodedUpload {
    uint8_t *host = nullptr, *dev = nullptr;
    bool pinned = false;
    bool queued = false;   // kernels queued behind the call's wait read `dev`
    size_t in_bytes = 0, table_offset = 0, table_bytes = 0, upload_bytes = 0;
    // the sizes: a packet of total_bytes whose directory starts at directory_offset, and its streams' blocks
    CodedUpload(uint64_t total_bytes, uint64_t directory_offset, const k::EntropyStreams &st)
        : in_bytes((size_t)(total_bytes - directory_offset)), table_offset((in_bytes + 7) & ~(size_t)7), table_bytes(8u * (size_t)st.total_blocks),
          upload_bytes(round256(table_offset + table_bytes)) {}
    CodedUpload(const CodedUpload &) = delete;
    // both buffers, and where the entropy stage reads the packet and its block table
    bool alloc(size_t extra, k::EntropyDecode &d) {
        host = (uint8_t *)host_alloc(upload_bytes, &pinned);
        d.in = dev = (uint8_t *)pool_alloc(upload_bytes + extra);
        d.block_at = (const uint32_t *)(dev + table_offset);
        return host && dev;
    }
    // the packet's bytes and the table into the staging buffer, their copy and the zeroing of the stage's flags onto the stream
    bool send(const uint8_t *packet, uint64_t directory_offset, const EntropyStream *streams, const k::EntropyStreams &st, uint32_t *flags, size_t flag_bytes,
              hipStream_t stream) {
        memcpy(host, packet + directory_offset, in_bytes);
        stage_block_table(streams, st, packet, directory_offset, (uint32_t *)(host + table_offset));
        return hipMemcpyAsync(dev, host, table_offset + table_bytes, hipMemcpyHostToDevice, stream) == hipSuccess &&
               hipMemsetAsync(flags, 0, flag_bytes, stream) == hipSuccess;
    }
    // the call has waited for the stream: the copy has read the staging buffer
    void sent() {
        if (host) host_free(host, pinned);
        host = nullptr;
    }
    void release() {
        sent();
        if (queued) tctx().free_later(dev); else pool_free(dev);
        dev = nullptr;
    }
    ~CodedUpload() { release(); }
};

// A frame's leaves on the device as a decoder has them (RULE P's reference), what a delta packet names of it, and the event of the
// work that made it: a feed from another thread's stream waits for that event first.
struct InterRefDev {
    void *block = nullptr;
    k::InterLeavesDev leaves{nullptr, nullptr, nullptr, 0};
    InterReference meta;
    hipEvent_t ready = nullptr;
    ~InterRefDev() {
        if (ready) { (void)hipEventSynchronize(ready); event_put(ready); }
        if (block) pool_free(block);
    }
    static std::unique_ptr<InterRefDev> make(const CodecLayout &l) {
        std::unique_ptr<InterRefDev> r(new InterRefDev());
        const size_t n = l.nleaves, keys_bytes = round256(8 * n);
        uint8_t *block = (uint8_t *)pool_alloc(keys_bytes + 4 * n);
        if (!block) return nullptr;
        r->block = block;
        r->leaves = k::InterLeavesDev{(unsigned long long *)block, block + keys_bytes, block + keys_bytes + 3 * n, l.nleaves};
        r->meta.timestamp = l.timestamp;
        r->meta.nleaves = l.nleaves;
        r->meta.bits = l.bits;
        r->meta.colour_bits = l.colour_bits;
        memcpy(r->meta.mn, l.mn, 12);
        r->meta.side = l.side;
        return r;
    }
    // the work that filled the leaves has been queued on the stream
    bool published(hipStream_t stream) {
        ready = event_get();
        return ready && hipEventRecord(ready, stream) == hipSuccess;
    }
    void wait_on(hipStream_t consumer) const {
        if (ready && hipStreamWaitEvent(consumer, ready, 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipEventSynchronize(ready);
        }
    }
};

// `held` gives way to `next` (may be null); kernels queued on the calling thread's stream may still read the old leaves
inline void replace_reference(std::unique_ptr<InterRefDev> &held, std::unique_ptr<InterRefDev> next) {
    if (held) {
        tctx().free_later(held->block);
        held->block = nullptr;
    }
    held = std::move(next);
}

}  // namespace cwipc_amd
