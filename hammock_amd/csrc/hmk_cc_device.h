// hmk_cc_device.h -- the lock-free union-find k_components.hip and k_density.hip share (device code only).
// It hooks the LARGER root under the smaller with one compare-and-swap: parent[i] <= i always, a root is the minimum of its tree,
// and only roots are ever hooked, so the final parent[] names each vertex's smallest member whatever the order of the edges.  While
// a kernel unites, every access to parent[] is a relaxed atomic at agent scope: the L1 is per compute unit and the L2 per XCD, and a
// plain load may return a word another XCD has long replaced.  An atomic load may still return an old parent, but an old parent is
// an ancestor (parents are only ever replaced by ancestors, roots only by the CAS), so cc_find still climbs to the root of its tree;
// and a CAS that fails returns the word as it is now, from where the lane goes on.  No lane waits for another: cc_find follows
// strictly decreasing indices, and a CAS is tried again only after some other CAS on that word succeeded.
#ifndef HMK_CC_DEVICE_H
#define HMK_CC_DEVICE_H

#include <hip/hip_runtime.h>

namespace hmk {

namespace {

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v's tree, halving the path behind it (a non-root's parent is replaced by an ancestor: a root is never stored to)
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t v) {
    uint32_t p = cc_load(parent + v);
    while (p != v) {
        const uint32_t g = cc_load(parent + p);
        if (g != p) cc_store(parent + v, g);
        v = p;
        p = g;
    }
    return v;
}

// joins the trees of a and b; true: this lane's CAS hooked a root (the number of trees went down by one)
__device__ __forceinline__ bool cc_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return false;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return true;
        a = seen;   // hi was hooked by someone else meanwhile: `seen` is its parent now, an ancestor below hi
        b = lo;
    }
}

}  // namespace

}  // namespace hmk
#endif
