// pinned_report.hpp -- the host half of the pinned-word report.  A kernel publishes a small result into the calling thread's pinned
// 64-bit words under a sequence tag (the kernel half: block_scan.hpp and the final kernels); the host arms the words it expects,
// launches, waits or polls, and believes a value only under the tag it armed with.  Two layouts exist:
//   packed:  word = value | tag << 32               (the compaction, the floor partition, the RGB-D count, the codec's sort and entropy decode)
//   plain:   n 64-bit values, then one word == tag  (the ICP sums)
// No HIP type: a host test (tests/test_pinned_report_host.py, through tests/abi/pinned_report_host.cpp) compiles the same text with
// the host C++ compiler on a plain array.
#pragma once

#include <cstdint>

namespace cwipc_amd {

class PinnedReport {
public:
    PinnedReport(volatile unsigned long long *words, uint32_t &counter) : m_words(words), m_counter(counter) {}
    // Zero words [first, first + count) and take the next tag, which is never 0: a zeroed word can pass for no tag.
    uint32_t arm(int first, int count) {
        for (int i = 0; i < count; i++) m_words[first + i] = 0ull;
        return ++m_counter ? m_counter : ++m_counter;
    }
    // packed: has word i -- have all of [first, first + count) -- been published under `tag`?
    bool landed(uint32_t tag, int i) const { return (uint32_t)(m_words[i] >> 32) == tag; }
    bool landed(uint32_t tag, int first, int count) const {
        for (int i = 0; i < count; i++)
            if (!landed(tag, first + i)) return false;
        return true;
    }
    // plain: is the word behind the n values the tag itself?
    bool landed_plain(uint32_t tag, int n) const { return m_words[n] == (unsigned long long)tag; }
    uint32_t value(int i) const { return (uint32_t)m_words[i]; }
    unsigned long long raw(int i) const { return m_words[i]; }
    // what the kernel is handed
    unsigned long long *device() const { return const_cast<unsigned long long *>(m_words); }

private:
    volatile unsigned long long *m_words;
    uint32_t &m_counter;
};

}  // namespace cwipc_amd
