// The workgroup primitives of the kernels that walk, count and order things -- events, annotations, density, windows, activity,
// soundscape; retrieval, search, clustering, silhouette: scan, compaction, reductions, the bitonic sort in LDS and the unordered append.
// Ballots, shuffles and LDS words in a fixed order: no result depends on timing, except the positions wave_append hands out (below).
// Every thread of the workgroup must make a block_* call (barriers inside).  The prefix over more items than a workgroup holds, with its
// three kernels and their launcher, is prefix_count.h.
#pragma once
#include "common.h"

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

// op over the values of the WAVES * 64 threads, for an op that is exact under reordering (integer sums, maxima): wave_reduce, lane 0 of
// each wave stores wt[wave], one barrier, every thread folds the WAVES words in wave order.  NO barrier follows: wt (WAVES words the
// caller lends) must not be rewritten before the workgroup's next barrier -- a caller with reductions back to back gives each its own words.
template <int WAVES, typename T, typename Op>
static __device__ __forceinline__ T block_reduce(T v, Op op, T* wt) {
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) wt[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = wt[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = op(r, wt[w]);
    return r;
}

// Sum of the THREADS threads' values by the LDS tree red[tid] += red[tid + s], s = THREADS / 2 .. 1: the one form of every floating-point
// sum over a workgroup, whose order of additions is part of the result (T: double, or a vector of them).  red: THREADS words the caller
// lends; they may be reused as soon as the call returns.
template <int THREADS, typename T>
static __device__ __forceinline__ T block_tree_sum(T v, T* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

// Bitonic sort of a[0 .. np2) in LDS, np2 a power of two >= 2: afterwards no a[i + 1] is before(a[i + 1], a[i]).  The caller pads the
// tail beyond its real elements with a value that sorts last and puts a barrier between its last write and the call; one follows the last step.
template <int THREADS, typename T, typename Before>
static __device__ __forceinline__ void block_bitonic_sort(T* a, int np2, Before before) {
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (np2 >> 1); t += THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const T x = a[i], y = a[j];
                if (before(y, x) == ((i & size) == 0)) {
                    a[i] = y;
                    a[j] = x;
                }
            }
            __syncthreads();
        }
}

// The lanes of a wave with `sel` append `value` to the list dst[0 .. cap) in LDS: a ballot, ONE atomicAdd on *fill for the wave, the
// popcount below the lane.  Every lane of the wave must make the call.  *fill counts every selected lane; one that lands at or beyond
// cap is not stored.  Which wave gets which range depends on timing: the list is a set in no order, and callers sort it afterwards.
template <typename T>
static __device__ __forceinline__ void wave_append(bool sel, T value, T* dst, int* fill, int cap) {
    const int lane = threadIdx.x & 63;
    const unsigned long long bal = __ballot(sel);
    if (bal == 0ull) return;      // wave-uniform
    int at = 0;
    if (lane == 0) at = atomicAdd(fill, (int)__popcll(bal));
    at = __shfl(at, 0) + (int)__popcll(bal & ((1ull << lane) - 1ull));
    if (sel && at < cap) dst[at] = value;
}
