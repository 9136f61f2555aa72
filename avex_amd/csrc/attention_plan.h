// Which kernel an attention call gets: avx::attention's dispatch as a pure function of (T, B, H, has bias table, CU count, knobs).
// Standard headers only (tests/test_dispatch_cpu.py builds it with the host compiler); attention.hip / attention16.hip launch from the plan.
#pragma once
#include <stddef.h>
#include <stdint.h>

void avexhip_set_error(const char* fmt, ...);

namespace avx {

constexpr int ATT_PLAN_TMAX = 512;      // variants 1 and 3 are built for T <= 512 (variant 3's nine-tile form: up to 544 keys)
// dynamic LDS of the kernels (attention.hip / attention16.hip assert that their layouts come to the same bytes)
constexpr int ATT_PLAN_LDS1 = 150816, ATT_PLAN_LDS2 = 152352, ATT_PLAN_LDS2L = 158496, ATT_PLAN_LDS2X = 150304, ATT_PLAN_LDS3 = 153376, ATT_PLAN_LDS3X = 152352;

// the environment's knobs as values; attention.hip's att_knobs() reads them, all per launch (tests and A/B runs switch them inside one process)
struct AttKnobs {
    int variant = 3;        // AVEX_AMD_ATT_VARIANT: 1 = stage-then-compute, 2 = persistent streamed (32x32x16 MFMAs), 3 = persistent streamed on 16x16x32 MFMAs (default up to 512 tokens)
    int grid = 0;           // AVEX_AMD_ATT_GRID > 0: workgroups (tests: several units per workgroup)
    int tail_rows = 2;      // AVEX_AMD_ATT_TAIL_ROWS: the longest last query block that goes to the tail kernel (tests raise it to 32)
    bool no_tail = false;   // AVEX_AMD_ATT_NO_TAIL set
    bool no_xt = false;     // AVEX_AMD_ATT_NO_XT set: no nine-tile forms
};

enum AttKernel { ATT_KERNEL1 = 1, ATT_KERNEL2 = 2, ATT_KERNEL3 = 3 };      // attention_kernel<T>, attention2_kernel<T, LONG, BIAS, XT>, attention3_kernel<T, BIAS, XT>

struct AttPlan {
    int rc = 0;                  // -1 (AVEXHIP_ERR_INVALID): refused, the text went to avexhip_set_error
    int variant = 3;
    AttKernel kernel = ATT_KERNEL3;
    bool k_long = false, k_bias = false, k_xt = false;      // the instantiation
    int nqb_main = 1;            // query blocks of 512 per (clip, head) item in the main kernel
    int per_block = 1;           // consecutive units per workgroup
    unsigned grid = 0; int block = 512; int lds = 0;
    bool use_tail = false;       // the last 1 .. 32 query rows in attention_tail_kernel<T, RW>
    int tail_rows = 0, tail_rw = 0; unsigned tail_grid = 0; size_t tail_lds = 0;
};

inline AttPlan plan_attention(int Tn, int B, int H, bool bias, int n_cu, const AttKnobs& k) {
    AttPlan p;
    p.variant = Tn > ATT_PLAN_TMAX ? 2 : k.variant;
    p.k_bias = bias;
    const int n_wg = k.grid > 0 ? k.grid : n_cu;
    const auto deal = [&](int64_t n_units) {      // (clip, head, query block) units, dealt to the workgroups in consecutive runs
        p.per_block = (int)((n_units + n_wg - 1) / n_wg);
        p.grid = (unsigned)((n_units + p.per_block - 1) / p.per_block);
    };
    if (p.variant == 3) {
        deal((int64_t)B * H);
        p.lds = ATT_PLAN_LDS3;
        return p;
    }
    if (p.variant != 2) {
        p.kernel = ATT_KERNEL1; p.grid = (unsigned)(B * H); p.block = 1024; p.lds = ATT_PLAN_LDS1;
        return p;
    }
    // A last query block of one or two rows (EAT's class token: 513 = 512 + 1) goes to the tail kernel instead of a further query block
    // of the streamed kernel.  Only that: in a short last block the waves without query rows skip their tiles, so the block is cheap
    // -- measured at 3 072 (clip, head) items (scripts/att_513.py): 513 tokens 0.441 ms with the tail, 0.491 without; 520 tokens
    // 0.532 / 0.485; 544 tokens 0.949 / 0.491 (and 1.79 ms with round 2's one-row-per-wave tail up to 32 rows).
    const int rem = Tn % 512;
    p.k_long = Tn > ATT_PLAN_TMAX;
    p.use_tail = p.k_long && rem > 0 && rem <= k.tail_rows && rem <= 32 && !k.no_tail;
    p.nqb_main = p.k_long ? (p.use_tail ? Tn / 512 : (Tn + 511) / 512) : 1;
    if (!((int64_t)B * H * p.nqb_main < (1ll << 31))) { avexhip_set_error("attention: too many (item, query block) units"); p.rc = -1; return p; }
    deal((int64_t)B * H * p.nqb_main);
    p.kernel = ATT_KERNEL2;
    if (!p.k_long) { p.lds = ATT_PLAN_LDS2; return p; }
    if (!bias && p.use_tail && p.nqb_main == 1 && Tn <= ATT_PLAN_TMAX + 32 && k.variant != 2 && !k.no_xt) {
        // EAT's shape (513 .. 544 tokens, no bias table, the rows beyond 512 in the tail kernel): the main block on variant 3's nine-tile form
        p.kernel = ATT_KERNEL3; p.k_long = false; p.k_xt = true; p.lds = ATT_PLAN_LDS3X;
    } else if (bias) {
        p.lds = ATT_PLAN_LDS2L;
    } else if (Tn % 256 >= 1 && Tn % 256 <= 32 && !k.no_xt) {
        // the 1 .. 32 keys beyond a multiple of 256 ride in the last full key block's phase as a ninth key tile (EAT: 513 keys)
        p.k_xt = true; p.lds = ATT_PLAN_LDS2X;
    } else {
        p.lds = ATT_PLAN_LDS2L;
    }
    if (p.use_tail) {
        if (!((int64_t)B * H * rem < (1ll << 31))) { avexhip_set_error("attention: too many tail rows"); p.rc = -1; return p; }
        // rows per wave: as many as the tail has (up to 8) and as fit the LDS (RW x (Tn + 64) floats)
        int rw = rem >= 8 ? 8 : (rem >= 4 ? 4 : (rem >= 2 ? 2 : 1));
        while (rw > 1 && sizeof(float) * (size_t)rw * ((size_t)Tn + 65 + 256) > 150 * 1024) rw >>= 1;
        p.tail_rows = rem; p.tail_rw = rw;
        p.tail_lds = sizeof(float) * (size_t)rw * ((size_t)Tn + 65 + 256);      // scores, q, gate, four partial output rows
        p.tail_grid = (unsigned)(B * H * ((rem + rw - 1) / rw));
    }
    return p;
}

}  // namespace avx
