// Two workgroup primitives the event, annotation, density, window and activity kernels share: a scan over the threads of a workgroup
// and the compaction of a range into the list of its kept members.  Both are integer work on ballots and shuffles, no atomics: their
// results do not depend on timing.  Every thread of the workgroup must make the call (barriers inside).
#pragma once
#include "common.h"

struct BlockSum {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// Scan of the WAVES * 64 threads' values in thread order under an associative `op` (op(a, b): a comes from the threads BELOW; it need
// not commute), `id` its identity.  Returns the thread's inclusive value, *excl = the composition of the threads below it, *total = of
// all threads.  wt: WAVES words of LDS the caller lends; they may be reused as soon as the call returns.
template <int WAVES, typename T, typename Op>
static __device__ __forceinline__ T block_scan(T v, T id, Op op, T* wt, T* excl, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(incl, o, 64);
        if (lane >= o) incl = op(t, incl);
    }
    T below = __shfl_up(incl, 1, 64);
    if (lane == 0) below = id;
    if (lane == 63) wt[wave] = incl;
    __syncthreads();
    T before = id, all = id;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before = op(before, wt[w]);
        all = op(all, wt[w]);
    }
    __syncthreads();                                  // wt may be rewritten by the caller's next pass
    *excl = op(before, below);
    *total = all;
    return op(before, incl);
}

// One workgroup of THREADS walks i = 0 .. n - 1, THREADS at a time: kept[] receives the i with keep(i), in increasing order, *count their
// number.  Ballot + popcount inside a wave, the wave totals through LDS, the count of the passes before in `carry`: a kept member's
// position is the number of kept members in front of it, so the list is in increasing order whatever the timing.
template <int THREADS, typename Keep>
static __device__ __forceinline__ void block_compact(int n, Keep keep, int* __restrict__ kept, int* __restrict__ count) {
    __shared__ int wave_total[THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += THREADS) {
        const int i = base + threadIdx.x;
        const bool k = i < n && keep(i);
        const unsigned long long m = __ballot(k);
        if (lane == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int q = 0; q < THREADS / 64; ++q) {
            const int t = wave_total[q];
            before += q < wave ? t : 0;
            total += t;
        }
        if (k) kept[carry + before] = i;
        carry += total;
        __syncthreads();                              // wave_total is rewritten by the next pass
    }
    if (threadIdx.x == 0) *count = carry;
}
