// The argument block of avx::gemm, in a header of its own: the kernels take it by value (common.h includes this file), and the planner
// (gemm_plan.h) reads it with no HIP header in sight, so a plain host compiler can build and test the dispatch.
// avx::gemm does not launch from the block it is given: plan_gemm() copies it, applies the launcher's rewrites to the copy (variant 8 -> 5,
// gelu 1 -> 6 for a half-only output, rows_out -> stats_out + ln_rowstats, tile_order / nt) and the kernel receives that copy.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace avx {

struct GemmArgs {
    const void* A; int64_t lda;
    const void* W; int64_t ldw;
    int M, N, K;
    const float* bias;
    const float* resid; int64_t ldr; float alpha;
    const void* resid_half; int64_t ldrh;   // residual in the operand type (used when resid == NULL)
    int gelu;
    float* out_f32; int64_t ldo;
    void* out_half; int64_t ldh;
    float* out_raw; int64_t ldraw;
    const uint8_t* row_zero;  // optional [M] mask: a row with a non-zero byte takes 0 in place of acc + bias -- its raw tap is 0.0 and its other outputs are what the
                              // rest of the epilogue makes of 0: resid * alpha through the activation, i.e. zeros when there is no residual (the one caller, the
                              // projection behind the patch embedding, has none); every kernel form that knows the mask does the same
    float half_scale;         // 0 or 1: off.  Otherwise out_half receives value * half_scale (a power of two: the third rung of the f16 range ladder stores
                              // fc1's hidden activations scaled down and folds the inverse into fc2's weights); generic epilogues only, fp32 outputs unscaled
    int variant;
    // ---- LayerNorm folded into the GEMMs around it (256-tile streaming kernel) --------------------------------------
    // A tensor y that is only ever consumed through LayerNorm is kept RAW in the operand type.  The GEMM that produces y writes
    // per-row partial statistics [M][N/64][2] = (sum, sum of squares) of each 64-column segment (stats_out); avx::ln_rowstats
    // reduces them, in a fixed order, to one (rstd, -mu * rstd) pair per row; the consumers take those pairs:
    //  * consumer of LN(y) as its A operand:  A = y, W = W * diag(gamma) (folded by the caller), ln_s[n] = sum_k W'[n][k],
    //    bias = b + W beta;  the epilogue forms  rstd[m] * acc + ((-mu rstd)[m] * ln_s[n] + bias[n])  before GELU / rounding;
    //  * consumer of LN(y) as its residual:  out = alpha * ((y * rstd - mu rstd) * gamma + beta) + acc + bias;
    //  * producer: stats_out receives the partial statistics of the rows it writes (from the fp32 values before rounding).
    const float* ln_rows;     // consumer-as-A: [M rounded up to 256][2] (rstd, -mu * rstd) of the A rows, or NULL
    const float* ln_s;        // [N]
    const void* lnr_y;        // consumer-as-residual: raw residual rows (half), or NULL
    int ldy;
    const float* lnr_rows;    // [M][2] (rstd, -mu * rstd) of the residual rows
    const float* lnr_gamma;   // [N]
    const float* lnr_beta;    // [N]
    int lnr_prefolded;        // lnr_gamma holds alpha * gamma and lnr_beta holds alpha * beta + bias (what the kernel takes; avx::lnr_fold makes them).
                              // avx::gemm folds per launch when the flag is clear; callers that launch the same fold repeatedly keep the vectors
    float* stats_out;         // [M][N/64][2] or NULL
    // The finished row statistics instead of (or beside) the partial ones: rows_out[m] = (rstd, -mu rstd) of output row m with rows_eps inside
    // the root -- what avx::ln_rowstats makes of stats_out, same bits: avx::gemm writes the partials to stats_out (required, as scratch) and
    // launches ln_rowstats itself.  Readable / writable up to M rounded up to even.
    float* rows_out; float rows_eps;
    // Mean-pooled hook tap without the tap: the rows are clips of pool_T (>= 64) consecutive rows; each 64-row block writes the column
    // sums of acc + bias (what out_raw would hold) over its rows, split at the one clip boundary it can contain:
    // pool_part[block][slot][N], slot 0 = the clip of the block's first row, slot 1 = the next clip.  avx::pool_reduce adds a clip's
    // blocks in order and divides by pool_T.  256-tile kernel, generic epilogue.
    float* pool_part; int pool_T;
    int pool_mode;            // 0: column sums (mean after pool_reduce); 1: column maxima; 2: each clip's FIRST row, written straight to pool_part = [clips][N]
    // 0, or the number of leading output columns that exist in memory (a multiple of 4, < N): the product is computed for N (a multiple of
    // the tile width, W and bias padded by the caller) but rows of every output / residual are only n_store wide.  128-tile kernels.
    int n_store;
    // skinny kernel (variant 7): A[m][k] *= a_scale[(m / a_scale_rows) * a_scale_ld + k] (fp32 product rounded to the operand type) as the rows
    // are loaded: a per-(clip, channel) rescale of the input without a pass of its own (EfficientNet's squeeze-excitation)
    const float* a_scale; int a_scale_rows; int a_scale_ld;
    // 128-tile LDS-DMA kernel: scratch for split-K (fp32 partial products [S][M][N]), or NULL.  With it a product of <= 64 tiles and
    // K >= 1024 is split S <= 8 ways along K and finished by splitk_epilogue_kernel (partials added in order).
    float* splitk_ws; size_t splitk_bytes;
    // A LayerNorm of the output rows y (after bias / residual) in the same pass: the workspace path above with an epilogue kernel that owns
    // whole rows (one wave per row, N <= 1024, N % 256 == 0, no activation): post_ln_out_* = LN(y) * post_ln_w + post_ln_b; y itself still
    // goes to out_f32 / out_half when those are set.  post_ln_round: y is rounded to the operand type before the statistics -- what a
    // LayerNorm kernel reading a half residual stream sees.  For the few-row products of one to eight clips, where a kernel less per
    // LayerNorm is 13 us less (avx::gemm_post_ln_ok says whether a product qualifies).
    const float* post_ln_w; const float* post_ln_b; float post_ln_eps; int post_ln_round;
    float* post_ln_out_f32; int64_t post_ln_ldo; void* post_ln_out_half; int64_t post_ln_ldh;
    // sticky range alarm: the number of (lane, launch) pairs that rounded at least one |value| > 65504 to an f16 output is added
    // here (one atomic per wave at most, at the end of the kernel); NULL = not counted.  bf16 outputs cannot overflow.
    unsigned int* ovf;
    int tile_order;           // 256-tile kernel: 0 = grouped walk where K < 2048 (default), 1 = row-major, >= 2 = grouped walk with that many row panels per group
    int nt;                   // set by the launcher: bit 0 non-temporal output stores (256-tile kernels)
};

}  // namespace avx
