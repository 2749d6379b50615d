// grx_unionfind.h -- the lock-free union-find of grx_biconnected.hip (connected components, then the components of
// the tree edges) and grx_components.hip (connected and weakly connected components): hook the larger root under the
// smaller with atomicCAS, pointer jumping while finding.  Device code only; int32 ids.
#pragma once
#include "grx_common.h"

// words other workgroups update while this kernel runs are read and written past the L1
__device__ __forceinline__ int grx_ld32(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void grx_st32(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// union-find with p[x] <= x: the root of a set is its smallest member that was ever hooked under nothing.  A vertex
// that has a parent keeps one for good, and every value ever stored in p[x] is a member of x's set below x, so a
// stale read only lengthens the walk.
__device__ __forceinline__ int grx_uf_find(int32_t *p, int x)
{
    int cur = grx_ld32(p + x);
    if (cur != x) {
        int prev = x, next;
        while (cur > (next = grx_ld32(p + cur))) {           // pointer jumping: prev skips cur
            grx_st32(p + prev, next);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

__device__ __forceinline__ void grx_uf_union(int32_t *p, int a, int b)
{
    int ra = grx_uf_find(p, a), rb = grx_uf_find(p, b);
    while (ra != rb) {
        if (ra < rb) { const int t = ra; ra = rb; rb = t; }
        const int old = atomicCAS(p + ra, ra, rb);           // hooks ra under the smaller rb only while ra is a root
        if (old == ra) break;
        ra = old;                                            // ra got a parent meanwhile: go on from there
    }
}

// every label to its root: after it p[v] is the smallest member of v's set
__device__ __forceinline__ void grx_uf_flatten(int32_t *p, int v)
{
    int r = v, next;
    while ((next = grx_ld32(p + r)) != r) r = next;
    grx_st32(p + v, r);
}
