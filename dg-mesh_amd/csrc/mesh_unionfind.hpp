// Lock-free union-find by minimum, shared by mesh_clean.hip (components through shared vertices) and mesh_repair.hip (components of
// the faces' double cover): parent[v] <= v always, parent[v] only ever decreases, and a root (parent[r] == r) is only ever changed
// by a compare-and-swap that expects r -- the single-pass form of ECL-CC (Jaiganesh & Burtscher, HPDC 2018): a link is made root to
// root by CAS, so no link is ever lost and no second round is needed.  After the hooking launch has ended, the root of every node
// is the smallest node of its component.
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so inside a hooking launch
// `parent` is read with agent-scope atomic loads and written with agent-scope atomics only.  Were a read stale all the same, it
// would return an older, larger ancestor of the same node: the chase still descends strictly, a CAS on a node that is no longer a
// root fails against the true value and the link is retried from the value it returned.
// Nothing waits: every loop names the monotone quantity that ends it.
#pragma once
#include "dgm_common.hpp"

#define AGENT __HIP_MEMORY_SCOPE_AGENT

namespace {

__device__ __forceinline__ int ld_parent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, AGENT); }

// The root of v's tree, halving the path on the way (parent[v] = min(parent[v], grandparent)).
__device__ __forceinline__ int find_root(int* parent, int v) {
    int p = ld_parent(parent + v);
    // ends: p = parent[v] < v strictly on every step that does not return (parent[x] <= x always), so v descends towards 0
    while (p != v) {
        const int g = ld_parent(parent + p);
        if (g != p) __hip_atomic_fetch_min(parent + v, g, __ATOMIC_RELAXED, AGENT);
        v = p;
        p = g;
    }
    return v;
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
    int ra = find_root(parent, a), rb = find_root(parent, b);
    // ends: ra + rb decreases strictly on every pass that does not break: a failed CAS returned old < hi, and the root found from
    // old is <= old.  A CAS fails only because another thread has made progress (it lowered parent[hi]): lock-free, nothing waits.
    while (ra != rb) {
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, AGENT)) break;
        ra = find_root(parent, expected);  // (expected now holds parent[hi] < hi)
        rb = lo;
        rb = find_root(parent, rb);
    }
}

// The root of v in a table that no longer changes (a launch after the hooking launch).
__device__ __forceinline__ int settled_root(const int* __restrict__ parent, int v) {
    int p = parent[v];
    // ends: p = parent[v] < v strictly until the root
    while (p != v) {
        v = p;
        p = parent[v];
    }
    return v;
}

}  // namespace
