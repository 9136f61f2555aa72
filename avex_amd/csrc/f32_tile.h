// The fp32 product of the evaluation metrics: a 128 x 128 x 32 tile of A B^T on v_mfma_f32_32x32x2_f32 (fp32 operands, one rounding per
// product), shared by retr_sim_kernel (retrieval.hip), srch_sim_kernel (search.hip) and clus_assign_kernel (clustering.hip), with the small
// helpers those files use around it.  Not for the f16 GEMM or the attention kernels: their tiles and staging differ.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(1))) const void gptr_t;
typedef __attribute__((address_space(3))) void lptr_t;

constexpr int FT_BM = 128, FT_BN = 128, FT_BK = 32;      // FT_BK fp32 = one 128-B LDS row = 8 chunks of 16 B
constexpr int FT_TILE_BYTES = 128 * FT_BK * 4;           // 16 KiB per operand tile
constexpr int FT_LDS_BYTES = 4 * FT_TILE_BYTES;          // dynamic LDS of a launch: two operands, double-buffered

static inline int64_t dpad_of(int d) { return ((int64_t)d + FT_BK - 1) / FT_BK * FT_BK; }
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// floats per row of a stored similarity matrix over n columns (retrieval.hip, search.hip)
static inline int64_t ldsim_of(int64_t n) { return (n + 63) / 64 * 64; }

// order-preserving map of a float onto unsigned integers (-0 is folded onto +0 first by the caller), and its inverse
static __device__ __forceinline__ unsigned mono32(float v) {
    const unsigned u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
static __device__ __forceinline__ float mono32_inv(unsigned u) { return __uint_as_float((u >> 31) ? u ^ 0x80000000u : ~u); }

// The rank key of retrieval, search, few-shot examples, k-means relocation and the density exemplars: (mono32(v) << 32) | (0xFFFFFFFF - index).
// Unsigned 64-bit order = value descending, then index ascending, so a maximum is "the best, the first on ties"; keys of different
// indices differ, and 0 is "no key" (no real key is 0: index < 2^32 - 1).  The caller passes v + 0.0f, which folds -0 onto +0; NaN
// sorts above +inf unless the caller drops it.  The high word may be any unsigned value instead of a float (density: a count).
static __device__ __forceinline__ unsigned rank_key_low(unsigned index) { return 0xFFFFFFFFu - index; }      // the low word; its own inverse
static __device__ __forceinline__ unsigned long long rank_key(unsigned hi, unsigned index) {
    return ((unsigned long long)hi << 32) | (unsigned long long)rank_key_low(index);
}
static __device__ __forceinline__ unsigned long long rank_key(float v, unsigned index) { return rank_key(mono32(v), index); }
// the same key from a low word the caller made with rank_key_low and kept (examples.hip holds a tile's in LDS)
static __device__ __forceinline__ unsigned long long rank_key_from_low(float v, unsigned low) {
    return ((unsigned long long)mono32(v) << 32) | (unsigned long long)low;
}
static __device__ __forceinline__ unsigned rank_key_index(unsigned long long key) { return rank_key_low((unsigned)(key & 0xFFFFFFFFull)); }
static __device__ __forceinline__ float rank_key_value(unsigned long long key) { return mono32_inv((unsigned)(key >> 32)); }

// acc = A[a0 .. a0 + 128) . B[b0 .. b0 + 128)^T for a workgroup of 256 threads with FT_LDS_BYTES of dynamic LDS.  A (na rows) and B (nb rows)
// are row-major with dpad floats per row (dpad % 32 == 0, zero beyond the real width).  Wave (wr, wc) = (wid >> 1, wid & 1) owns rows
// [64 wr, +64) x columns [64 wc, +64) of the tile as 2 x 2 MFMA tiles, acc[i][j] at (32 i, 32 j) of that block; f32_tile_row / f32_tile_col
// name its elements.  Operands are staged by LDS-DMA into a double buffer with the chunk swizzle of gemm_nt_kernel (gemm.hip), one barrier
// per K tile; every thread of the workgroup must make the call.  v_mfma_f32_32x32x2_f32 takes ONE float per lane and operand: lane
// (i = lane & 31, h = lane >> 5) supplies row i at k-index h.  A lane reads 4 consecutive floats (one swizzled 16-B chunk, chunk 2 kk + h)
// and feeds them to 4 MFMAs; both operands use the same k assignment, so the order of the sum inside a K tile is permuted, not its terms.
static __device__ __forceinline__ void f32_tile_product(const float* A, int na, int a0, const float* B, int nb, int b0, int dpad,
                                                        f32x16 (&acc)[2][2]) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int nk = dpad / FT_BK;

    auto stage_dma = [&](int st, int k0) __attribute__((always_inline)) {
        char* abase = smem + st * (2 * FT_TILE_BYTES);
        char* bbase = abase + FT_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rloc = wid * 32 + i * 8 + (lane >> 3);
            const int chunk = (lane & 7) ^ ((rloc >> 1) & 7);
            int arow = a0 + rloc, brow = b0 + rloc;
            arow = arow < na ? arow : na - 1;      // rows past the end repeat the last one; the caller does not use their results
            brow = brow < nb ? brow : nb - 1;
            const float* asrc = A + (int64_t)arow * dpad + k0 + chunk * 4;
            const float* bsrc = B + (int64_t)brow * dpad + k0 + chunk * 4;
            const int dst = (wid * 32 + i * 8) * 128;      // wave-uniform; hardware adds lane * 16
            __builtin_amdgcn_global_load_lds((gptr_t*)asrc, (lptr_t*)(abase + dst), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t*)bsrc, (lptr_t*)(bbase + dst), 16, 0, 0);
        }
    };
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int st) __attribute__((always_inline)) {
        const char* abase = smem + st * (2 * FT_TILE_BYTES);
        const char* bbase = abase + FT_TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            f32x4 af[2], bf[2];
            const int chunk = 2 * kk + (lane >> 5);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = wr * 64 + i * 32 + (lane & 31);
                af[i] = *(const f32x4*)(abase + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int row = wc * 64 + j * 32 + (lane & 31);
                bf[j] = *(const f32x4*)(bbase + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
    };

    stage_dma(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my DMA pieces of tile kt have landed
        __syncthreads();                                      // everyone's landed; everyone finished reading buffer (kt + 1) & 1
        if (kt + 1 < nk) stage_dma((kt + 1) & 1, (kt + 1) * FT_BK);
        compute(kt & 1);
    }
}

// Row and column, within the 128 x 128 tile, of acc[i][j][reg] of the calling thread (C/D layout of the 32x32 MFMA forms inside the wave's
// 64 x 64 block).  The 32 lanes of a half wave hold the 32 columns of one row.
static __device__ __forceinline__ int f32_tile_row(int i, int reg) {
    const int lane = threadIdx.x & 63, wr = threadIdx.x >> 7;
    return wr * 64 + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
}
static __device__ __forceinline__ int f32_tile_col(int j) {
    const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) & 1;
    return wc * 64 + j * 32 + (lane & 31);
}

// The bodies of the two kernels that retrieval.hip and search.hip both run, written once so that "the same arithmetic" is the same code.
//
// Rows for the product, one wave per row and 4 rows per workgroup of 256 threads: out[row] = dpad floats, zero beyond d; divided by
// max(||row||_2, 1e-12) in fp32 when `normalise`, copied when not.
static __device__ __forceinline__ void f32_prepare_rows(const float* __restrict__ x, int64_t ldx, int n, int d, int dpad, bool normalise,
                                                        float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* r = x + (int64_t)row * ldx;
    if (!normalise) {
        float* o = out + (int64_t)row * dpad;
        for (int c = lane; c < dpad; c += 64) o[c] = c < d ? r[c] : 0.f;
        return;
    }
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) ss = __builtin_fmaf(r[c], r[c], ss);
    float nrm = __builtin_sqrtf(wave_sum(ss));
    nrm = nrm < 1e-12f ? 1e-12f : nrm;
    float* o = out + (int64_t)row * dpad;
    for (int c = lane; c < dpad; c += 64) o[c] = c < d ? r[c] / nrm : 0.f;
}

// S[q][n] = Q[q] . D[n] for the 128 x 128 tile (blockIdx.y, blockIdx.x) of q in [0, nq), n in [0, nd): f32_tile_product with a store.  Q and
// D are prepared rows of dpad floats; S has lds_ floats per row.  The launch needs FT_LDS_BYTES of dynamic LDS.
static __device__ __forceinline__ void f32_tile_store_product(const float* __restrict__ Q, int nq, const float* __restrict__ D, int nd, int dpad,
                                                              float* __restrict__ S, int64_t lds_) {
    const int n0 = blockIdx.x * FT_BN, q0 = blockIdx.y * FT_BM;
    f32x16 acc[2][2];
    f32_tile_product(Q, nq, q0, D, nd, n0, dpad, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + f32_tile_col(j);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = q0 + f32_tile_row(i, r);
                if (q < nq && n < nd) S[(int64_t)q * lds_ + n] = acc[i][j][r];
            }
        }
}

}  // namespace
