// tk_wave_search.h -- the 64-ary wave search shared by the packed-rows kernels (tk_seqpack.hip) and the join kernel
// (tk_join.hip): "which document / part holds stream position g".
#ifndef TK_WAVE_SEARCH_H
#define TK_WAVE_SEARCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// Entries of the non-decreasing a[0 .. n) that are <= key.  The whole wave calls it with the same arguments: every step the
// 64 lanes probe the last entries of 64 equal parts of the range and a ballot keeps the one part the answer lies in.
// Ties are fine (tk_seqpack.hip passes a strictly increasing array, tk_join.hip one with runs of equal entries): all the search
// needs is that "a[p] <= key" holds on a prefix of the array and nowhere else.  The probes go up with the lane, so the ballot is
// a prefix of the lanes, c of them.  c < 64: probe c - 1 was not clamped to hi - 1 (a clamped probe is repeated by every later
// lane, which would make c = 64), so the entries up to lo + c * step - 1 hold, and the first probe that fails, at pc, bounds the
// answer from above.  The answer is therefore also the index of the LAST entry <= key, plus one.
__device__ __forceinline__ uint64_t tks_wave_count_le(const uint64_t* a, uint64_t n, uint64_t key) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t lo = 0, hi = n;                            // the answer is in [lo, hi]
    while (hi > lo) {
        const uint64_t step = (hi - lo + 63u) / 64u;
        uint64_t p = lo + (lane + 1u) * step - 1u;
        if (p >= hi) p = hi - 1u;
        const uint32_t c = (uint32_t)__builtin_popcountll(__ballot(a[p] <= key));   // a prefix of the lanes
        if (c == 64u) { lo = hi; break; }
        uint64_t pc = lo + (c + 1u) * step - 1u;        // the first probe above key: the answer is at most its index
        if (pc >= hi) pc = hi - 1u;
        lo += c * step;
        hi = pc;
    }
    return lo;
}

#endif
