// Which kernel a product gets: the GEMM dispatch as a pure host function.  plan_gemm() decides everything avx::gemm decides -- the
// rewrites of the argument block, the kernel family and its template instantiation, grid / block / LDS bytes, the split count, the
// kernels that follow, or the refusal -- and launches nothing; gemm.hip's execute() is a switch from the plan to the launch lines.
// Standard headers and GemmArgs only: tests/test_dispatch_cpu.py builds this file with the host compiler and checks the plans.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gemm_args.h"

void avexhip_set_error(const char* fmt, ...);

namespace avx {

// ---- tile geometry (gemm.hip asserts that its kernels were built for the same numbers) --------------------------------------------
constexpr int PLAN_BM = 128, PLAN_BN = 128, PLAN_BK = 64;      // 128-tile kernels
constexpr int PLAN_T2 = 256;                                   // 256-tile streaming kernel
constexpr int PLAN_LDS128 = 2 * 2 * 128 * PLAN_BK * 2;         // two stages of two 16 KiB operand tiles
constexpr int PLAN_LDS256 = 2 * (2 * PLAN_T2 * PLAN_BK * 2) + 32768;
constexpr int PLAN_OK = 0, PLAN_INVALID = -1;                  // AVEXHIP_OK, AVEXHIP_ERR_INVALID

// ---- environment knobs, as values.  gemm.hip's gemm_knobs() is the one place that reads the variables -----------------------------
struct GemmKnobs {
    bool variant_set = false; int variant = 0;      // AVEX_AMD_GEMM_VARIANT (per launch): set at all -> no automatic skinny choice; non-zero -> the variant of a variant-0 product
    bool skinny = true;                             // AVEX_AMD_GEMM_SKINNY != 0 (per launch)
    bool generic = false;                           // AVEX_AMD_GEMM_GENERIC != 0 (per launch)
    int grid = 0;                                   // AVEX_AMD_GEMM_GRID (per launch), >= 8: workgroups of the streaming kernel
    int tile_order = 0;                             // AVEX_AMD_GEMM_TILE_ORDER (per launch)
    int nt = 1;                                     // AVEX_AMD_GEMM_NT (once per process)
    int min_tiles = 128;                            // AVEX_AMD_GEMM_256_MIN_TILES (once per process)
    bool post_ln = true;                            // AVEX_AMD_POST_LN != 0 (per call)
    int lds_pad = 0;                                // AVEX_AMD_DEBUG_LDS_PAD (once per process)
};

// ---- the rules, one copy each ------------------------------------------------------------------------------------------------------
inline bool gemm_skinny_dim(int d) { return d == 32 || d == 64 || d == 96 || d == 128 || d == 160 || d == 256; }
// the skinny kernel's shapes: W [N, K] resident in LDS
inline bool gemm_skinny_shape(int K, int N) { return gemm_skinny_dim(K) && gemm_skinny_dim(N) && N * K <= 32768; }
// may a caller lay its activations out for the skinny kernel (and force variant 7)?  Off with AVEX_AMD_GEMM_SKINNY=0 or any AVEX_AMD_GEMM_VARIANT
inline bool gemm_rule_skinny_takes(int K, int N, const GemmKnobs& k) { return k.skinny && !k.variant_set && gemm_skinny_shape(K, N); }
// does the skinny kernel take this product?  (half output only, no fp32 / raw outputs, no folded LayerNorm, no row mask)
inline bool gemm_skinny_ok(const GemmArgs& a) {
    if (!gemm_skinny_shape(a.K, a.N)) return false;
    if (!a.out_half || a.out_f32 || a.resid || a.row_zero || a.ln_rows || a.lnr_y || a.stats_out || a.pool_part) return false;
    if (a.half_scale != 0.f && a.half_scale != 1.f) return false;
    if (a.lda % 8 || a.ldw % 8 || a.ldh % 8 || (a.resid_half && a.ldrh % 8) || (a.out_raw && a.ldraw % 4) || (a.n_store > 0 && a.n_store % 16)) return false;
    return true;
}
// a variant-0 product long and thin enough for the skinny kernel (before the knobs have their say)
inline bool gemm_skinny_auto(const GemmArgs& a) {
    return a.variant == 0 && a.M >= 32768 && a.K % 64 == 0 && (a.N == 64 || a.N % 128 == 0) && !a.out_raw && gemm_skinny_ok(a);
}
// the choice for a plain product (variant 0, no folded LayerNorm, no pooled tap): the 256-tile streaming kernel wants enough tiles to
// occupy the chip: from about half a tile per CU it wins (K = 768 -> N = 2304 at 3 968 rows, 144 tiles: 26 us against 41), below that
// the 128-tile kernel does -- four times the tiles, split-K for long contractions (K = 3072 -> N = 768 at 3 968 rows, 48 tiles: 44 us
// against 66; scripts/gemm_midsize.py, profiles/r03r_midsize.txt)
inline bool gemm_rule_streams(int M, int N, const GemmKnobs& k) {
    const int t256 = ((M + PLAN_T2 - 1) / PLAN_T2) * (N / PLAN_T2);
    return N % PLAN_T2 == 0 && M >= 1024 && t256 >= k.min_tiles;
}
// can the streaming kernel take this product at all?  (a product sent to it that it cannot take goes to the 128-tile kernel)
inline bool gemm_rule_streaming_takes(const GemmArgs& a) {
    return !(a.K < 2 * PLAN_BK || a.N % PLAN_T2 != 0 || (a.out_half && a.ldh % 8) || (a.resid_half && a.ldrh % 8));
}
// whether a product (M, N, K set; splitk_ws lent) can take GemmArgs::post_ln_*
inline bool gemm_rule_post_ln_ok(const GemmArgs& a, const GemmKnobs& k) {
    return k.post_ln && a.splitk_ws && a.N % 256 == 0 && a.N <= 1024 && a.K % PLAN_BK == 0 && !a.gelu && !a.ln_rows && !a.lnr_y && !a.stats_out && !a.pool_part &&
           !(a.n_store > 0 && a.n_store < a.N) && (size_t)a.M * a.N * sizeof(float) <= a.splitk_bytes && !gemm_rule_streams(a.M, a.N, k) &&
           (a.variant == 0 || a.variant == 3);
}

// The skinny kernel's instantiations gemm_skinny_kernel<T, NT = N / 16, KS = K / 32, SCALE, RAW>: each pair without and with the A-row
// scale; the raw fp32 tap exists for the projection widths (NT = 2, 4, 8, 16) in one form, with the scale
#define AVX_SKINNY_SHAPES(X) \
    X(4, 1) X(8, 1) X(4, 2) X(4, 4) X(4, 8) X(8, 2) X(8, 4) X(8, 8) X(16, 2) X(16, 4) \
    X(6, 2) X(4, 3) X(8, 3) X(10, 2) X(4, 5) X(8, 5)      /* EfficientNet's 96- and 144 (-> 160)-channel expansions */ \
    X(2, 1) X(2, 2) X(2, 3) X(2, 4) X(2, 5) X(2, 8) X(6, 1) X(10, 1) X(16, 1)      /* ... and its 16- and 24-channel block outputs kept at 32 channels in memory */
constexpr bool gemm_skinny_has_raw(int nt) { return nt == 2 || nt == 4 || nt == 8 || nt == 16; }
inline bool gemm_skinny_has(int nt, int ks) {
#define AVX_SK_HAS(NTV, KSV) if (nt == NTV && ks == KSV) return true;
    AVX_SKINNY_SHAPES(AVX_SK_HAS)
#undef AVX_SK_HAS
    return false;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
enum GemmFamily { GEMM_REFUSED = 0, GEMM_SKINNY, GEMM_STREAM, GEMM_TILE128_REG, GEMM_TILE128_DMA };
enum GemmAfter { GEMM_AFTER_NONE = 0, GEMM_AFTER_SPLITK, GEMM_AFTER_SPLITK_LN };

struct GemmPlan {
    int rc = PLAN_OK;            // PLAN_INVALID: refused, the text went to avexhip_set_error; nothing else in the plan counts
    GemmArgs args;               // as the kernel receives them
    GemmFamily family = GEMM_REFUSED;
    int epi = 0, ln = 0, act = 0;                                          // GEMM_STREAM: gemm256p_kernel<T, EPI, LN, ACT>
    int sk_nt = 0, sk_ks = 0; bool sk_scale = false, sk_raw = false;       // GEMM_SKINNY: gemm_skinny_kernel<T, NT, KS, SCALE, RAW>
    unsigned grid_x = 0, grid_y = 1; int block = 0; size_t lds = 0;
    int S = 1;                   // GEMM_TILE128_DMA: K splits (= grid_y)
    bool fold_lnr = false;       // args.lnr_gamma / lnr_beta are still the caller's: execute() folds them per launch (avx::lnr_fold) in stream-ordered scratch
    float* rows_out = nullptr;   // non-null: avx::ln_rowstats(args.stats_out -> rows_out) follows the product
    GemmAfter after = GEMM_AFTER_NONE; unsigned after_grid = 0;            // splitk_epilogue_kernel / splitk_ln_epilogue_kernel (256 threads)
};

#define AVX_PLAN_CHECK(cond, ...) do { if (!(cond)) { avexhip_set_error(__VA_ARGS__); return PLAN_INVALID; } } while (0)
#define AVX_PLAN_REQUIRE(cond, ...) do { if (!(cond)) { avexhip_set_error(__VA_ARGS__); p.rc = PLAN_INVALID; p.family = GEMM_REFUSED; return p; } } while (0)

// avx::gemm's own argument checks (before the CU count is asked for and anything is planned)
inline int gemm_validate(const GemmArgs& a) {
    AVX_PLAN_CHECK(a.A && a.W, "gemm: A and W must be non-null");
    AVX_PLAN_CHECK(a.M > 0 && a.N > 0 && a.K > 0, "gemm: empty problem M=%d N=%d K=%d", a.M, a.N, a.K);
    AVX_PLAN_CHECK(a.N % PLAN_BN == 0 || ((a.variant == 7 || (a.variant == 0 && a.N == 64 && a.M >= 32768 && a.K % 64 == 0)) && gemm_skinny_ok(a)),
                   "gemm: N=%d must be a multiple of %d (64 columns: the skinny streaming kernel only, >= 32768 rows)", a.N, PLAN_BN);
    AVX_PLAN_CHECK(a.K % PLAN_BK == 0 || (a.K % 32 == 0 && a.variant == 7), "gemm: K=%d must be a multiple of %d (of 32 with the skinny kernel, variant 7)", a.K, PLAN_BK);
    AVX_PLAN_CHECK(a.lda % 8 == 0 && a.ldw % 8 == 0, "gemm: lda/ldw must be multiples of 8 elements");
    AVX_PLAN_CHECK(a.half_scale == 0.f || a.half_scale == 1.f || (a.out_half && !a.stats_out && !a.post_ln_w && !a.pool_part && a.variant != 7 && a.half_scale > 0.f),
                   "gemm: half_scale goes with a plain half output (no row statistics, folded post-LayerNorm, pooled tap or skinny kernel)");
    AVX_PLAN_CHECK(a.out_f32 || a.out_half || a.out_raw || (a.post_ln_w && (a.post_ln_out_f32 || a.post_ln_out_half)), "gemm: no output buffer");
    AVX_PLAN_CHECK((!a.out_f32 || a.ldo % 4 == 0) && (!a.out_half || a.ldh % 4 == 0) &&
                       (!a.out_raw || a.ldraw % 4 == 0) && (!a.resid || a.ldr % 4 == 0) &&
                       (!a.resid_half || a.ldrh % 4 == 0),
                   "gemm: output/residual leading dims must be multiples of 4 elements");
    return PLAN_OK;
}

inline GemmPlan plan_gemm(const GemmArgs& in, int n_cu, const GemmKnobs& k) {
    GemmPlan p;
    p.args = in;
    GemmArgs& a = p.args;
    // GELU whose only consumer reads the operand type: the degree-4 fit, in whichever kernel and epilogue form runs (activation code 6)
    if (a.gelu == 1 && a.out_half && !a.out_f32) a.gelu = 6;
    if (a.lnr_y && !a.lnr_prefolded) {
        // the kernel takes alpha * gamma and bias + alpha * beta: callers that launch the same fold repeatedly keep those vectors
        // (lnr_prefolded); for the others execute() makes them
        AVX_PLAN_REQUIRE(a.lnr_gamma && a.lnr_beta && a.bias, "gemm: lnr_y needs lnr_gamma, lnr_beta and bias");
        p.fold_lnr = true;
        a.lnr_prefolded = 1;
    }
    if (a.variant == 8) a.variant = 5;      // the number of a removed full-row kernel that gave variant 5's bits: another name of variant 5
    AVX_PLAN_REQUIRE(!a.a_scale || ((a.variant == 7 || a.variant == 1) && a.a_scale_rows > 0 && a.a_scale_ld >= a.K && a.a_scale_ld % 4 == 0),
                     "gemm: a_scale is built for the skinny kernel (variant 7) and the register-staged 128-tile kernel (variant 1)");
    // variant 7 / auto for long thin products: the skinny streaming kernel (W resident in LDS, A rows straight into MFMA operands)
    if (a.variant == 7) AVX_PLAN_REQUIRE(gemm_skinny_ok(a), "gemm: variant 7 (skinny) takes K in {32, 64, 96, 128, 160, 256}, N in {32, 64, 96, 128, 160, 256} with N K <= 32768, a half output (N=%d K=%d)", a.N, a.K);
    if (a.variant == 7 || (gemm_skinny_auto(a) && (a.N % PLAN_BN != 0 || (k.skinny && !k.variant_set)))) {
        p.sk_nt = a.N / 16; p.sk_ks = a.K / 32;
        AVX_PLAN_REQUIRE(gemm_skinny_has(p.sk_nt, p.sk_ks), "gemm: no skinny instantiation for N=%d K=%d", a.N, a.K);
        AVX_PLAN_REQUIRE(!a.out_raw || (gemm_skinny_has_raw(p.sk_nt) && a.a_scale), "gemm: the skinny kernel writes a raw tap only for N = 32 / 64 / 128 / 256 with a_scale (N=%d)", a.N);
        p.family = GEMM_SKINNY;
        p.sk_scale = a.a_scale != nullptr; p.sk_raw = a.out_raw != nullptr;
        p.lds = (size_t)p.sk_nt * 16 * p.sk_ks * 32 * 2;
        const int64_t nblk = ((int64_t)a.M + 127) / 128;
        int per_cu = (int)(128 * 1024 / (p.lds > 16384 ? p.lds : 16384));      // workgroups per CU the LDS (and ~100 registers per lane) allows
        per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
        const int64_t grid = (int64_t)n_cu * per_cu;
        p.grid_x = (unsigned)(grid < nblk ? grid : nblk); p.block = 256;
        return p;
    }
    if (a.rows_out) {
        // no kernel below finishes the row statistics: partials to stats_out, then ln_rowstats
        AVX_PLAN_REQUIRE(a.stats_out, "gemm: rows_out needs stats_out as scratch");
        p.rows_out = a.rows_out;
        a.rows_out = nullptr;
    }
    // variant: 0 = auto, 1 = 128-tile register staging, 3 = 128-tile LDS-DMA, 5 (or 2, its tile-per-workgroup ancestor's number) =
    // the 256-tile streaming kernel
    int variant = a.variant;
    if (a.ln_rows || a.lnr_y || a.stats_out) {
        // folded LayerNorm exists in the 256-tile kernel only
        AVX_PLAN_REQUIRE(a.N % PLAN_T2 == 0 && a.K >= 2 * PLAN_BK && (!a.out_half || a.ldh % 8 == 0), "gemm: folded LayerNorm needs N %% 256 == 0 and K >= 128 (N=%d K=%d)", a.N, a.K);
        AVX_PLAN_REQUIRE(!a.ln_rows || (a.ln_s && a.bias && a.M >= 2), "gemm: ln_rows needs ln_s and bias");
        AVX_PLAN_REQUIRE(!a.lnr_y || (a.lnr_rows && a.lnr_gamma && a.lnr_beta && a.bias && a.lnr_prefolded && a.ldy % 8 == 0 && !a.resid && !a.resid_half),
                         "gemm: lnr_y needs lnr_rows / gamma / beta / bias and no other residual");
        AVX_PLAN_REQUIRE(a.variant == 0 || a.variant == 2 || a.variant == 5, "gemm: folded LayerNorm is built for the 256-tile kernel only");
        variant = 5;
    }
    if (a.n_store > 0 && a.n_store < a.N) {      // narrow outputs: the 128-tile kernels only
        AVX_PLAN_REQUIRE(a.n_store % 4 == 0 && !a.ln_rows && !a.lnr_y && !a.stats_out && !a.pool_part, "gemm: n_store=%d needs a multiple of 4 and no folded LayerNorm / pooled tap", a.n_store);
        if (variant == 0 || variant == 2 || variant == 5) variant = 3;
    }
    if (a.pool_part) {
        AVX_PLAN_REQUIRE(a.pool_T >= 64 && a.pool_mode >= 0 && a.pool_mode <= 2, "gemm: pool_part needs clips of at least 64 rows (got %d) and pool_mode 0..2 (got %d)", a.pool_T, a.pool_mode);
        AVX_PLAN_REQUIRE((a.variant == 0 || a.variant == 2 || a.variant == 5) && a.N % PLAN_T2 == 0 && a.K >= 2 * PLAN_BK, "gemm: pool_part is built for the 256-tile kernel only");
        variant = 5;
    }
    if (variant == 0) variant = k.variant;
    if (variant == 0) variant = gemm_rule_streams(a.M, a.N, k) ? 5 : 3;
    if (a.post_ln_w) variant = 3;      // (the caller checked gemm_post_ln_ok)
    if (variant == 2) variant = 5;
    if (variant == 5 && !gemm_rule_streaming_takes(a)) variant = 3;
    if (variant == 5) {
        const int tiles = ((a.M + PLAN_T2 - 1) / PLAN_T2) * (a.N / PLAN_T2);
        a.tile_order = k.tile_order;
        a.nt = ((k.nt & 4) && a.N <= 768) ? 0 : (k.nt & 1);      // AVEX_AMD_GEMM_NT: 0 no hints, 1 (default) non-temporal output stores, 5 = only for outputs wider than 768 columns (diagnostics)
        int grid = tiles < n_cu ? ((tiles + 7) / 8) * 8 : (n_cu / 8) * 8;
        if (grid < 8) grid = 8;
        if (k.grid >= 8) grid = (k.grid / 8) * 8;      // tests: force many tiles per workgroup
        p.family = GEMM_STREAM;
        p.grid_x = (unsigned)grid; p.block = 512; p.lds = PLAN_LDS256;
        const bool scaled = a.half_scale != 0.f && a.half_scale != 1.f;      // the fast epilogues do not know GemmArgs::half_scale
        // (k.generic -- tests: cross-check of the fast epilogues)
        const bool plain_out = a.out_half && a.bias && !a.out_f32 && !a.out_raw && !a.pool_part && !a.resid && !a.row_zero && !k.generic && !scaled;
        const bool fast_half = plain_out && !a.resid_half && !a.lnr_y && !a.stats_out && (a.gelu <= 2 || a.gelu == 6);      // the fast epilogue knows GELU and SiLU only
        const bool fast_resid = plain_out && (a.resid_half || a.lnr_y) && !a.gelu && !a.ln_rows;
        if (fast_half) {
            p.epi = 1; p.ln = a.ln_rows ? 1 : 0;
            p.act = (a.gelu == 1 || a.gelu == 6) ? 1 : (a.gelu == 2 ? 2 : 0);      // (half output only: 1 and 6 both mean the degree-4 fit here)
        } else if (fast_resid) {
            p.epi = 2; p.ln = (a.lnr_y ? 1 : 0) | (a.stats_out ? 2 : 0);
        } else if (a.pool_part) {
            p.epi = 0; p.ln = a.pool_mode + 1;
        }
        return p;
    }
    const int tiles = ((a.M + PLAN_BM - 1) / PLAN_BM) * (a.N / PLAN_BN);
    p.grid_x = (unsigned)tiles; p.block = 256; p.lds = (size_t)PLAN_LDS128 + k.lds_pad;
    if (variant == 1) { p.family = GEMM_TILE128_REG; return p; }
    p.family = GEMM_TILE128_DMA;
    // split-K when the caller lent a workspace and the product is few tiles of a long contraction (one clip's fc2: 24 tiles, K = 3072)
    if (a.post_ln_w) AVX_PLAN_REQUIRE(gemm_rule_post_ln_ok(a, k), "gemm: post_ln_* needs the 128-tile kernel's workspace path (N %% 256 == 0, N <= 1024, no activation, splitk_ws >= M N floats)");
    if (a.splitk_ws && (a.K >= 1024 || a.post_ln_w)) {
        p.S = 8;      // as many splits as keep the launch within two workgroups per CU (and leave every split at least two K-steps)
        while (p.S > 1 && (tiles * p.S > 2 * n_cu || a.K % (p.S * PLAN_BK) != 0 || a.K / p.S < 2 * PLAN_BK || (size_t)p.S * a.M * a.N * sizeof(float) > a.splitk_bytes)) p.S >>= 1;
    }
    p.grid_y = (unsigned)p.S;
    if (a.post_ln_w) { p.after = GEMM_AFTER_SPLITK_LN; p.after_grid = (unsigned)((a.M + 3) / 4); }
    else if (p.S > 1) { p.after = GEMM_AFTER_SPLITK; p.after_grid = (unsigned)(((int64_t)a.M * (a.N / 4) + 255) / 256); }
    return p;
}
#undef AVX_PLAN_CHECK
#undef AVX_PLAN_REQUIRE

}  // namespace avx
