// pinned_report_host.cpp -- the host half of the pinned-word report (csrc/pinned_report.hpp) as a stand-alone host program on a plain
// array that stands in for the pinned words, for tests/test_pinned_report_host.py (built with -fsanitize=address,undefined: the array
// is exactly as long as the words it stands for, so a step outside it ends the program).
//   pinned_report_host CHECK      one of the checks below; prints what does not hold and returns 1, else prints "ok" and returns 0
#include "pinned_report.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace cwipc_amd;

namespace {

int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            failures++;                                                 \
        }                                                               \
    } while (0)

constexpr int NWORDS = 32;   // ThreadCtx::host_words: 64 pinned 32-bit words
constexpr unsigned long long FILL = 0xa5a5a5a5deadbeefull;

unsigned long long packed(uint32_t value, uint32_t tag) { return (unsigned long long)value | ((unsigned long long)tag << 32); }

void arming_zeroes_its_range_only() {
    for (int first = 0; first < NWORDS; first++)
        for (int count = 0; first + count <= NWORDS; count++) {
            std::vector<unsigned long long> words(NWORDS, FILL);
            uint32_t counter = 7;
            PinnedReport report(words.data(), counter);
            const uint32_t tag = report.arm(first, count);
            EXPECT(tag == 8 && counter == 8);
            for (int i = 0; i < NWORDS; i++) EXPECT(words[i] == (i >= first && i < first + count ? 0ull : FILL));
        }
}

void tags_count_up_and_skip_zero() {
    std::vector<unsigned long long> words(NWORDS, FILL);
    uint32_t counter = 0;
    PinnedReport report(words.data(), counter);
    EXPECT(report.arm(0, 1) == 1);
    EXPECT(report.arm(0, 1) == 2);
    EXPECT(report.arm(3, 2) == 3 && counter == 3);
    counter = 0xfffffffeu;
    EXPECT(report.arm(0, 1) == 0xffffffffu && counter == 0xffffffffu);
    EXPECT(report.arm(0, 1) == 1 && counter == 1);   // never 0: a zeroed word would pass for it
    EXPECT(report.arm(0, 1) == 2);
    // a second report over the same counter goes on where the first stopped (ThreadCtx::report() builds one per call)
    PinnedReport again(words.data(), counter);
    EXPECT(again.arm(0, 1) == 3 && counter == 3);
}

void packed_word_lands_under_its_tag_only() {
    std::vector<unsigned long long> words(NWORDS, FILL);
    for (uint32_t start : {0u, 41u, 0xfffffffeu, 0xffffffffu}) {
        uint32_t counter = start;
        PinnedReport report(words.data(), counter);
        const uint32_t previous = report.arm(5, 1);
        words[5] = packed(123, previous);
        EXPECT(report.landed(previous, 5));
        const uint32_t tag = report.arm(5, 1);
        EXPECT(tag != 0 && tag != previous);
        EXPECT(!report.landed(tag, 5));                       // the zero word
        words[5] = packed(123, previous);
        EXPECT(!report.landed(tag, 5));                       // the previous tag's word
        words[5] = packed(tag, 0);
        EXPECT(!report.landed(tag, 5));                       // the tag in the low half, nothing above
        words[5] = packed(tag, previous);
        EXPECT(!report.landed(tag, 5));                       // the tag in the low half under the previous tag
        words[5] = packed(tag, tag ^ 0x80000000u);
        EXPECT(!report.landed(tag, 5));                       // one bit of the tag off
        words[5] = packed(0, tag);
        EXPECT(report.landed(tag, 5) && report.value(5) == 0);   // the value 0 under the tag has landed
        words[5] = packed(0xffffffffu, tag);
        EXPECT(report.landed(tag, 5) && report.value(5) == 0xffffffffu);
        EXPECT(!report.landed(tag, 4) && !report.landed(tag, 6));   // the neighbours hold FILL
    }
}

void range_lands_when_every_word_has() {
    for (int count = 1; count <= 16; count++)
        for (int missing = -1; missing < count; missing++) {
            std::vector<unsigned long long> words(NWORDS, FILL);
            uint32_t counter = 99;
            PinnedReport report(words.data(), counter);
            const int first = 3;
            const uint32_t tag = report.arm(first, count);
            EXPECT(!report.landed(tag, first, count));
            for (int i = 0; i < count; i++)
                if (i != missing) words[first + i] = packed(1000 + i, tag);
            EXPECT(report.landed(tag, first, count) == (missing < 0));
            if (missing >= 0) {
                words[first + missing] = packed(1000 + missing, tag - 1);   // a stale word in the gap
                EXPECT(!report.landed(tag, first, count));
            }
            EXPECT(report.landed(tag, first, 0));   // nothing is asked of an empty range
        }
}

void plain_layout_wants_the_tag_word_exactly() {
    for (int n : {1, 16, 29, NWORDS - 1}) {
        std::vector<unsigned long long> words(NWORDS, FILL);
        uint32_t counter = 0xffffffffu;
        PinnedReport report(words.data(), counter);
        const uint32_t tag = report.arm(n, 1);   // the word behind the n values
        EXPECT(tag == 1);
        for (int i = 0; i < n; i++) EXPECT(words[i] == FILL);   // the values are the kernel's to write: arming left them
        EXPECT(words[n] == 0ull && !report.landed_plain(tag, n));
        words[n] = (unsigned long long)tag;
        EXPECT(report.landed_plain(tag, n));
        words[n] = (unsigned long long)tag | (1ull << 32);
        EXPECT(!report.landed_plain(tag, n));                   // the upper half must be zero
        words[n] = packed(0, tag);
        EXPECT(!report.landed_plain(tag, n));                   // the packed layout's word is not the plain one's
        words[n] = (unsigned long long)(tag + 1);
        EXPECT(!report.landed_plain(tag, n));
        words[n] = 0xffffffffull;                               // the previous tag
        EXPECT(!report.landed_plain(tag, n));
    }
}

void reads_return_the_written_bits() {
    std::vector<unsigned long long> words(NWORDS, 0);
    uint32_t counter = 0;
    PinnedReport report(words.data(), counter);
    const double sum = -1234.5678e-9;
    unsigned long long bits;
    memcpy(&bits, &sum, sizeof(bits));
    const unsigned long long samples[] = {0ull, 1ull, 0xffffffffull, 0x100000000ull, 0x8000000000000000ull, 0xffffffffffffffffull, FILL, bits};
    int i = 0;
    for (unsigned long long s : samples) words[i++] = s;
    i = 0;
    for (unsigned long long s : samples) {
        EXPECT(report.raw(i) == s);
        EXPECT(report.value(i) == (uint32_t)(s & 0xffffffffull));
        i++;
    }
    double back;
    const unsigned long long raw = report.raw(7);
    memcpy(&back, &raw, sizeof(back));
    EXPECT(memcmp(&back, &sum, sizeof(sum)) == 0);
    EXPECT(report.device() == words.data());   // what the kernel is handed is the words themselves
}

const struct { const char *name; void (*run)(); } CHECKS[] = {
    {"arming_zeroes_its_range_only", arming_zeroes_its_range_only},
    {"tags_count_up_and_skip_zero", tags_count_up_and_skip_zero},
    {"packed_word_lands_under_its_tag_only", packed_word_lands_under_its_tag_only},
    {"range_lands_when_every_word_has", range_lands_when_every_word_has},
    {"plain_layout_wants_the_tag_word_exactly", plain_layout_wants_the_tag_word_exactly},
    {"reads_return_the_written_bits", reads_return_the_written_bits},
};

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2)
        for (const auto &check : CHECKS)
            if (strcmp(argv[1], check.name) == 0) {
                check.run();
                if (failures == 0) printf("ok\n");
                return failures ? 1 : 0;
            }
    fprintf(stderr, "usage: pinned_report_host CHECK, one of:\n");
    for (const auto &check : CHECKS) fprintf(stderr, "  %s\n", check.name);
    return 2;
}
