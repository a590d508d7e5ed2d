// geo4d_amd/csrc/union_find.h — a lock-free union-find over int32 ids in device memory: find_root and union_min, for any kernel that
// produces edges between ids (mesh_components.hip today; a producer of voxel or point edges can use it as it stands).
//
// parent int32 [N] starts as the identity. The three invariants every operation keeps:
//   (1) parent[x] <= x, and parent[x] == x iff x is a root;
//   (2) a word only ever gets smaller: a root is lowered by one successful compare-and-swap (expected value: itself), a non-root by an
//       atomic minimum with one of its own ancestors; so a non-root never becomes a root again;
//   (3) parent[x] is in x's set: sets only ever merge.
// From (1) every chain x, parent[x], parent[parent[x]], .. strictly descends and ends at a root after at most x steps, whatever other
// threads write meanwhile, and the root of a finished set is its smallest id. No thread waits for another: there is no flag, lock or
// ticket, only loads, one atomic minimum and one compare-and-swap, each of which completes on its own.
//
// Every access is a relaxed agent-scope atomic: another XCD's L2 may hold an older line, and by (2) an older value is a larger one, still
// an ancestor-or-self in the same set: it costs a step or a retry, never a wrong answer.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's set as far as this thread can see, halving the path on the way (parent[x] := its grandparent, by atomic minimum).
// Terminates: p is parent[x] as loaded, p <= x by (1); a turn of the loop either ends it (p == x: a root) or goes on from x' = p < x
// with p' = the value loaded from parent[p]; ids are >= 0, so at most x turns.
__device__ __forceinline__ int find_root(int* parent, int x) {
    int p = uf_load(parent + x);
    while (p != x) {
        const int g = uf_load(parent + p);                                         // g <= p < x
        if (g != p) (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// join the sets of a and b, the larger root under the smaller; returns a member of the joined set at or near its root (a good place to
// start the next find from). Terminates: a turn either returns (one set already, or the swap took), or the swap failed
// because hi is no longer a root, and then the value it returned is hi's parent, < hi by (1) and (2): the next turn starts from
// (that, lo), a pair whose sum is strictly smaller; ids are >= 0 and find_root only lowers them further. Nothing waits.
__device__ __forceinline__ int union_min(int* parent, int a, int b) {
    // one parent for both: one set already, by (3), and no word of a root was read. Once most ids point at their root this is how most
    // calls end, and the few root words, which every find ends on, are left to the calls that have something to join.
    const int pa = uf_load(parent + a);
    if (pa == uf_load(parent + b)) return pa;
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return a;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const int seen = atomicCAS(parent + hi, hi, lo);                            // only a root is ever the target
        if (seen == hi) return lo;
        a = seen;                                                                   // < hi: somebody linked hi first
        b = lo;
    }
}

}  // namespace
