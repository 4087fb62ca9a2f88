// union_find_host.cpp -- csrc/union_find.hpp compiled for the host, run sequentially (tests/test_union_find_host.py).
//
//   union_find_host chain <n> <ascending|descending|shuffled> <seed>
//       n points on a chain, i linked to i + 1; the n - 1 unions issued in that order; then find(i) for every i.
//       prints: "labels_zero <0|1> steps <parent words loaded by every find, the unions' and the final ones>"
//   union_find_host forest <n> <m> <seed>
//       m random unions among n points, held against a plain sequential union-find (smallest index as the representative).
//       prints: "mismatches <count> invariant <0|1> steps <...>"
#include "union_find.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

using namespace cwipc_amd;

namespace {

struct HostAtomics {
    unsigned long long loads = 0;
    uint32_t load(const uint32_t *p) { loads++; return *p; }
    uint32_t fetch_min(uint32_t *p, uint32_t v) { const uint32_t old = *p; if (v < old) *p = v; return old; }
};

bool invariant_holds(const std::vector<uint32_t> &parent) {
    for (size_t i = 0; i < parent.size(); i++) if (parent[i] > i) return false;
    return true;
}

int chain(uint32_t n, const char *order, unsigned seed) {
    std::vector<uint32_t> parent(n), edge(n ? n - 1 : 0);
    std::iota(parent.begin(), parent.end(), 0u);
    std::iota(edge.begin(), edge.end(), 0u);
    if (!strcmp(order, "descending")) std::reverse(edge.begin(), edge.end());
    else if (!strcmp(order, "shuffled")) { std::mt19937 rng(seed); std::shuffle(edge.begin(), edge.end(), rng); }
    else if (strcmp(order, "ascending")) return 2;
    HostAtomics at;
    for (uint32_t e : edge) (void)uf_union(parent.data(), e + 1, e, at);   // the larger index first, as the link kernel calls it
    bool zero = invariant_holds(parent);
    for (uint32_t i = 0; i < n; i++) zero = zero && uf_find(parent.data(), i, at) == 0u;
    printf("labels_zero %d steps %llu\n", zero ? 1 : 0, at.loads);
    return 0;
}

int forest(uint32_t n, uint32_t m, unsigned seed) {
    std::vector<uint32_t> parent(n), plain(n);
    std::iota(parent.begin(), parent.end(), 0u);
    std::iota(plain.begin(), plain.end(), 0u);
    auto plain_find = [&](uint32_t x) { while (plain[x] != x) x = plain[x]; return x; };
    std::mt19937 rng(seed);
    HostAtomics at;
    bool inv = true;
    for (uint32_t e = 0; e < m; e++) {
        const uint32_t a = rng() % n, b = rng() % n;
        (void)uf_union(parent.data(), a, b, at);
        const uint32_t ra = plain_find(a), rb = plain_find(b);
        if (ra != rb) plain[std::max(ra, rb)] = std::min(ra, rb);
        if ((e & 255u) == 0u) inv = inv && invariant_holds(parent);
    }
    inv = inv && invariant_holds(parent);
    unsigned long long mismatches = 0;
    for (uint32_t i = 0; i < n; i++) mismatches += uf_find(parent.data(), i, at) != plain_find(i);
    printf("mismatches %llu invariant %d steps %llu\n", mismatches, inv ? 1 : 0, at.loads);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "chain")) return chain((uint32_t)atol(argv[2]), argv[3], (unsigned)atol(argv[4]));
    if (argc == 5 && !strcmp(argv[1], "forest")) return forest((uint32_t)atol(argv[2]), (uint32_t)atol(argv[3]), (unsigned)atol(argv[4]));
    fprintf(stderr, "usage: union_find_host chain n order seed | forest n m seed\n");
    return 2;
}
