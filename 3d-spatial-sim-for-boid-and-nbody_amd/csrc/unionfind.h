// The lock-free union-find shared by the group finders: nbmi_fof over key ranks (nbmi.hip) and bdmi_flocks over
// cell-sorted ranks (bdmi.hip).  Device code only; every function takes the arrays of its caller.  Three kernels in a
// row use it, and both finders have one of each: init (fof_init), link (fof_unite / fof_link_lanes), flatten (fof_flatten).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The state of rank r before the link kernel: a set of its own; minid / cnt are what fof_flatten's atomics start from.
__device__ __forceinline__ void fof_init(int64_t r, int32_t *__restrict__ parent, int32_t *__restrict__ minid,
                                         int32_t *__restrict__ cnt) {
    parent[r] = (int32_t)r;
    minid[r] = INT32_MAX;
    cnt[r] = 0;
}

// The union-find.  parent[] is int32 over ranks, parent[r] = r before the link kernel.  Invariants:
//   (a) A store only ever LOWERS parent[r] (a root is hooked under a smaller rank by a CAS, path halving is an atomic
//       min).  So parent[r] <= r always, every parent chain strictly decreases, and fof_find terminates even on stale
//       values - a stale parent is still an ancestor.
//   (b) Two roots are hooked only by CAS(&parent[hi], hi, lo) with lo < hi.  On failure the thread goes on from the
//       value the CAS returned: another thread has lowered that word, so the system as a whole always progresses.
//   (c) NO loop waits for another thread's progress: no spin, no flag, no barrier across waves.  Every iteration of
//       fof_find steps down a strictly decreasing chain; every iteration of fof_unite ends in a return or follows a
//       word that somebody lowered.
//   (d) During the link kernel EVERY access to parent[] is an agent-scope relaxed atomic (load, min, CAS): the eight
//       XCDs have private L2s and a CU's L1 is never refreshed by other CUs' stores (radix.hip's discipline for its
//       status words).  Plain accesses begin behind the next kernel boundary: the flatten kernel of either finder
//       (k_fof_flatten, k_fs_flatten), which reads parent[] through fof_flatten below.
__device__ __forceinline__ int fof_load(int32_t *parent, int r) {
    return __hip_atomic_load(parent + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int fof_find(int32_t *parent, int r) {
    int p = fof_load(parent, r);
    while (p != r) {
        const int g = fof_load(parent, p);
        if (g != p) (void)__hip_atomic_fetch_min(parent + r, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // path halving
        r = p;
        p = g;
    }
    return r;
}
// joins the sets of a and b; returns the root of the joined set as this thread saw it last (an ancestor of both from now on)
__device__ __forceinline__ int fof_unite(int32_t *parent, int a, int b) {
    for (;;) {
        a = fof_find(parent, a);
        b = fof_find(parent, b);
        if (a == b) return a;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return lo;
        a = seen;  // (< hi: whoever won the word lowered it)
        b = lo;
    }
}
// The lanes of a wave that found a link to the body of rank r (wave-uniform) at the same moment.  Every lane carries
// `mine`, an ancestor of its own rank (its rank at first, then whatever root it saw last): lanes with equal ancestors are
// in one set already, so of those that share the first linking lane's ancestor only that lane goes to memory, and the
// others take over the root it comes back with.  An optimisation only: every set that links to r is united with r.
// Called by all lanes that evaluated r (link = false for those that are too far), in one branch.
__device__ __forceinline__ void fof_link_lanes(int32_t *parent, bool link, int &mine, int r) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(link);
    if (m == 0ull) return;
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
    const int lane = threadIdx.x & 63;
    const int shared = __builtin_amdgcn_readlane(mine, leader);
    const bool follows = link && lane != leader && mine == shared;
    if (link && !follows) mine = fof_unite(parent, mine, r);
    const int joined = __builtin_amdgcn_readlane(mine, leader);
    if (follows) mine = joined;
}
// The kernel behind the link kernel, one lane per rank r (every lane of the wave calls it, r >= n included): parent[] is
// final and read plainly.  root[r] = the root of r's tree, minid[root] = the smallest caller index id_of(rank) and
// cnt[root] = the number of ranks below it (integer atomics: order independent).
// Adjacent ranks mostly share their root, and a root that a large group hangs on would otherwise take one same-address
// atomic per member: the lanes that share the root of the first lane left go in as one (twice), the rest on their own.
template <class IdOf>
__device__ __forceinline__ void fof_flatten(int64_t r, int64_t n, const int32_t *__restrict__ parent, int32_t *__restrict__ root,
                                            int32_t *__restrict__ minid, int32_t *__restrict__ cnt, IdOf id_of) {
    const bool valid = r < n;
    const int lane = threadIdx.x & 63;
    int f = -1, own = INT32_MAX;
    if (valid) {
        f = (int)r;
        for (int p = parent[f]; p != f; p = parent[f]) f = p;
        root[r] = f;
        own = id_of(r);
    }
    unsigned long long todo = __builtin_amdgcn_ballot_w64(valid);
    for (int round = 0; round < 2 && todo != 0ull; round++) {
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int f0 = __builtin_amdgcn_readlane(f, leader);
        const bool with = ((todo >> lane) & 1ull) != 0ull && f == f0;
        const unsigned long long same = __builtin_amdgcn_ballot_w64(with);
        int least = with ? own : INT32_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(least, o);
            least = other < least ? other : least;
        }
        if (lane == leader) {
            atomicMin(&minid[f0], least);
            atomicAdd(&cnt[f0], (int)__popcll(same));
        }
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) {
        atomicMin(&minid[f], own);
        atomicAdd(&cnt[f], 1);
    }
}
