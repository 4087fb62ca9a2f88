// union_find.hpp -- the atomic union-find over an array of parents: the marker detector's connected dark pixels (kernels_markers.hip)
// and the Euclidean clusters of a cloud (kernels_cluster.hip, RULE K of hip_ext.h).  No HIP type: the atomic load and the atomic
// minimum come in as a policy, so a host test (tests/test_union_find_host.py, through tests/abi/union_find_host.cpp) compiles the
// same text with the host compiler, runs it sequentially and counts its steps.  Under hipcc everything is inlined into the kernel.
//
//   policy:  uint32_t load(const uint32_t *p)                  the word, read atomically (every call counts as one STEP of a find)
//            uint32_t fetch_min(uint32_t *p, uint32_t v)       *p = min(*p, v) atomically; returns the word as it was
//
// INVARIANT.  parent[x] <= x for every x that takes part, at all times.  The caller starts with parent[x] = x, and the only two
// stores are fetch_min(&parent[a], b) with b < a (uf_union) and fetch_min(&parent[x], g) with g < x (uf_find's path halving).  So
// the word of an x only ever decreases, and a root -- parent[x] == x -- is the smallest index of everything that hangs under it.
//
// MEMBERSHIP.  Every value ever stored in parent[x] is a member of x's component (of the graph of all unions asked for).  A union
// stores b = the end of a walk from one side of a pair asked for, a itself being the end of the walk from the other side; halving
// stores g, read from parent[p] with p read from parent[x]: by induction over the stores both are members, and membership is
// transitive.  So no tree ever holds two components.
//
// uf_find TERMINATES whatever other lanes do: a step leaves with x when the word read is >= x (the root), with p when p's word is
// >= p, and otherwise goes on with g < p < x.  x is a non-negative integer and strictly decreases: at most x rounds.
//
// uf_union TERMINATES whatever other lanes do: a round returns, or replaces the larger of the pair (a, after the swap) by `old`,
// which the fetch_min read from parent[a] and which differs from a, hence is < a by the invariant; the finds never increase a or
// b.  So a + b strictly decreases from round to round and is bounded below by 0.
//
// CORRECTNESS, once every lane has returned (a kernel boundary): R(x), the root that x's chain of parents ends at, is the same for
// the two ends of every union asked for -- with MEMBERSHIP, the trees are exactly the components.  H(x) is the set of all values
// parent[x] ever held.  By induction over m the two statements hold together for every index <= m:
//   (history)  R(v) = R(x) for every v in H(x), x <= m.   H(x) = x > v1 > ... > vk, vk the final word, so R(vk) = R(x).  The store
//              that replaced v(i) by v(i+1), i >= 1, was a union's -- then that lane's fetch_min returned old = v(i) != x and it went
//              on with the pair (v(i), v(i+1)), both < x: by (pair) R(v(i)) = R(v(i+1)) -- or a halving's: v(i+1) = g was read from
//              parent[p], and p from parent[x], so p = v(j) with 1 <= j <= i and g is in H(p), p < x: R(g) = R(p) = R(v(j)).  Down
//              the chain all of v1 .. vk share one root.  (The store that replaced x by v1 is a union's: halving reads p < x first.)
//   (pair)     a union's loop that stands at (a, b), both <= m, ends with R(a) = R(b).   Induction over a + b.  The finds follow
//              words that were read, members of H: a' and b' with R(a') = R(a), R(b') = R(b) by (history).  a' == b': done.
//              Otherwise a' > b' after the swap and fetch_min(&parent[a'], b') returns old.  old == a': b' is in H(a') now,
//              R(b') = R(a').  old < a': old is in H(a'), R(old) = R(a'), and the loop stands at (old, b') with a smaller sum.
// Both use each other only at smaller indices or sums.  A lane that SKIPS a union because the other end's word equals a value it
// has read on its own chain (kernels_cluster.hip) relies on (history) alone.
//
// STALE LOADS are harmless.  Nothing above needs a load to return the word's latest value, only SOME value the word has held: such a
// value is < x or the root test's own x (termination), a member (MEMBERSHIP) and in H(x) (CORRECTNESS).  What decides a union is what
// fetch_min returns, and that is the word itself.
//
// PATH HALVING is required, not an optimisation: a component whose indices descend along a chain (point i linked to i - 1 only, the
// unions arriving in ascending order of i, as a cloud scanned along a line delivers them) costs n^2 / 2 dependent loads without it --
// harmless in a 1920-pixel image row, a launch that does not come back at 2 M points.  With it a sequential run of that chain takes
// under 5 n steps in any order of the unions (the host test holds 20 n).
#pragma once

#include <cstdint>

#ifndef CWIPC_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_HOST_DEVICE __host__ __device__
#else
#define CWIPC_HOST_DEVICE
#endif
#endif

#ifndef CWIPC_FORCEINLINE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWIPC_FORCEINLINE __forceinline__
#else
#define CWIPC_FORCEINLINE inline
#endif
#endif

namespace cwipc_amd {

// the root of x's tree, halving the path on the way
template <class Atomics>
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint32_t uf_find(uint32_t *parent, uint32_t x, Atomics &at) {
    for (;;) {
        const uint32_t p = at.load(parent + x);
        if (p >= x) return x;    // the root (or a word that is no index: the caller's "takes no part", left alone)
        const uint32_t g = at.load(parent + p);
        if (g >= p) return p;
        at.fetch_min(parent + x, g);
        x = g;
    }
}

// a and b in one tree; returns a member of that tree that was its root when the call looked (the smaller end)
template <class Atomics>
CWIPC_HOST_DEVICE CWIPC_FORCEINLINE uint32_t uf_union(uint32_t *parent, uint32_t a, uint32_t b, Atomics &at) {
    for (;;) {
        a = uf_find(parent, a, at);
        b = uf_find(parent, b, at);
        if (a == b) return a;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = at.fetch_min(parent + a, b);
        if (old == a) return b;   // a was a root and hangs below b now
        if (old > a) return b;    // (cannot happen, by the invariant; leaving keeps the loop's bound independent of it)
        a = old;
    }
}

#if defined(__HIPCC__)
// the device's policy: relaxed, agent scope -- the lanes of one kernel on one device; the kernel boundary publishes the result
struct UfDeviceAtomics {
    __device__ __forceinline__ uint32_t load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t fetch_min(uint32_t *p, uint32_t v) { return atomicMin(p, v); }
};
#endif

}  // namespace cwipc_amd
