// The exclusive prefix of one small integer per item, val(i) for i = 0 .. n - 1, by counting: per block of 1 024 items a sum, one workgroup
// over the block sums, then the rank inside the block -- three launches, no atomics, no host round trip.  density.hip numbers its clusters
// with it (the roots in the order of the lowest core row), regions.hip the set cells of each frame, the region roots and the kept regions
// (a compaction that keeps order).  A user brings
//   n() -> int64_t                 the number of items: PrefixHostN, or PrefixDevN where the count lives on the device alone
//   val(int64_t i) -> int or bool  what item i counts (>= 0)
//   Total                          int32_t or int64_t: the width of *total, the sum over all items
//   store(int64_t i, int rank, v)  what the last pass keeps of item i: rank = the sum of val below i, v = val(i)
// and a workspace of prefix_count_blocks(n) integers.  rank is exact modulo 2^32 (unsigned arithmetic, which wraps): a caller whose total
// may reach 2^31 takes Total = int64_t, reads *total and refuses the ranks.
#pragma once
#include "block_prims.h"

namespace {

constexpr int kPrefixBlock = 1024;                               // items per block: 256 threads, four consecutive items each

inline int64_t prefix_count_blocks(int64_t n) { return (n + kPrefixBlock - 1) / kPrefixBlock; }

// n = min(n_host, *n_dev) where the count lives on the device alone (n_dev not null); the grid follows n_host
__device__ __forceinline__ int64_t prefix_n(int64_t n_host, const int64_t* n_dev) {
    if (!n_dev) return n_host;
    const int64_t n = *n_dev;
    return n < n_host ? n : n_host;
}
struct PrefixHostN {
    int64_t n;
    __device__ __forceinline__ int64_t operator()() const { return n; }
};
struct PrefixDevN {
    int64_t n_host;
    const int64_t* n_dev;
    __device__ __forceinline__ int64_t operator()() const { return prefix_n(n_host, n_dev); }
};

struct PrefixStoreRank {         // out[i] = rank, for every item
    int32_t* out;
    __device__ __forceinline__ void operator()(int64_t i, int rank, int) const { out[i] = rank; }
};

template <typename N, typename V>
__global__ __launch_bounds__(256) void prefix_count_kernel(N n_of, V val, int32_t* __restrict__ block) {
    __shared__ int wt[4];
    const int64_t n = n_of();
    const int64_t b0 = (int64_t)blockIdx.x * kPrefixBlock + 4 * threadIdx.x;
    int c = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (b0 + e < n) c += val(b0 + e);
    int before, all;
    block_scan<4>(c, 0, BlockSum(), wt, &before, &all);
    if (threadIdx.x == 0) block[blockIdx.x] = all;
}

// one workgroup: block[b] -> the sum of the blocks before b (its low 32 bits), *total = all
template <typename Total>
__global__ __launch_bounds__(256) void prefix_blocks_kernel(int64_t n_blocks, int32_t* __restrict__ block, Total* __restrict__ total) {
    __shared__ Total part[256];
    const int tid = threadIdx.x;
    const int64_t per = (n_blocks + 255) / 256;
    const int64_t lo = per * tid, hi = lo + per < n_blocks ? lo + per : n_blocks;      // (hi < lo behind the last block: no trip)
    Total s = 0;
    for (int64_t b = lo; b < hi; ++b) s += block[b];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        Total run = 0;
        for (int k = 0; k < 256; ++k) {
            const Total v = part[k];
            part[k] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    Total run = part[tid];
    for (int64_t b = lo; b < hi; ++b) {
        const int v = block[b];
        block[b] = (int32_t)(uint32_t)(uint64_t)run;
        run += v;
    }
}

template <typename N, typename V, typename Store>
__global__ __launch_bounds__(256) void prefix_apply_kernel(N n_of, V val, const int32_t* __restrict__ block, Store store) {
    __shared__ int wt[4];
    const int64_t n = n_of();
    const int64_t b0 = (int64_t)blockIdx.x * kPrefixBlock + 4 * threadIdx.x;
    decltype(val(b0)) v[4];      // (int, or bool where an item counts 0 or 1)
    int c = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = b0 + e < n ? val(b0 + e) : 0;
        c += v[e];
    }
    int before, all;
    block_scan<4>(c, 0, BlockSum(), wt, &before, &all);          // the items of the threads below this one
    int run = (int)((unsigned)block[blockIdx.x] + (unsigned)before);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (b0 + e < n) {
            store(b0 + e, run, v[e]);
            run = (int)((unsigned)run + (unsigned)v[e]);
        }
}

// the three launches over a grid for n_host >= 1 items.  block: prefix_count_blocks(n_host) integers of workspace
template <typename Total, typename N, typename V, typename Store>
int prefix_count(int64_t n_host, N n_of, V val, int32_t* block, Total* total, Store store, hipStream_t s) {
    const int64_t n_blocks = prefix_count_blocks(n_host);
    prefix_count_kernel<N, V><<<dim3((unsigned)n_blocks), dim3(256), 0, s>>>(n_of, val, block);
    AVX_LAUNCH_CHECK();
    prefix_blocks_kernel<Total><<<dim3(1), dim3(256), 0, s>>>(n_blocks, block, total);
    AVX_LAUNCH_CHECK();
    prefix_apply_kernel<N, V, Store><<<dim3((unsigned)n_blocks), dim3(256), 0, s>>>(n_of, val, block, store);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

}  // namespace
