// Prints the plan of every product / attention call described on stdin, one line each (tests/test_dispatch_cpu.py).  Host C++ only: the
// planner headers, no HIP, no library.
//
//   gemm M=496 N=768 K=3072 out_half bias splitk_ws=8 GEMM_GRID=16 cu=256
//   att T=513 B=2 H=12 bias ATT_NO_XT=1
//   ask M=496 N=768 K=3072 out_half splitk_ws=8          (the callers' queries for that product)
//
// `name=value` sets an integer field, a bare pointer name lends a dummy buffer, an upper-case name is a knob (the environment variable
// without its AVEX_AMD_ prefix).  Leading dimensions default to the dense ones; splitk_ws=n lends n * M * N floats.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>

#include "../../avex_amd/csrc/attention_plan.h"
#include "../../avex_amd/csrc/gemm_plan.h"

static char g_err[512];
void avexhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static float g_buf[16];      // every lent pointer: never dereferenced by a planner

static void gemm_line(std::istringstream& in, bool ask) {
    avx::GemmArgs a;
    memset(&a, 0, sizeof(a));
    avx::GemmKnobs k;
    int n_cu = 256;
    long splitk_n = -1;
    a.A = g_buf; a.W = g_buf;
    std::string tok;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        const std::string key = tok.substr(0, eq);
        const long v = eq == std::string::npos ? 0 : atol(tok.c_str() + eq + 1);
#define INT_FIELD(f) if (key == #f) { a.f = (decltype(a.f))v; continue; }
        INT_FIELD(M) INT_FIELD(N) INT_FIELD(K) INT_FIELD(variant) INT_FIELD(gelu) INT_FIELD(n_store) INT_FIELD(pool_T) INT_FIELD(pool_mode)
        INT_FIELD(lda) INT_FIELD(ldw) INT_FIELD(ldh) INT_FIELD(ldo) INT_FIELD(ldraw) INT_FIELD(ldr) INT_FIELD(ldrh) INT_FIELD(ldy)
        INT_FIELD(a_scale_rows) INT_FIELD(a_scale_ld) INT_FIELD(lnr_prefolded)
#undef INT_FIELD
#define PTR_FIELD(f) if (key == #f) { a.f = (decltype(a.f))g_buf; continue; }
        PTR_FIELD(bias) PTR_FIELD(resid) PTR_FIELD(resid_half) PTR_FIELD(out_f32) PTR_FIELD(out_half) PTR_FIELD(out_raw) PTR_FIELD(row_zero)
        PTR_FIELD(ln_rows) PTR_FIELD(ln_s) PTR_FIELD(lnr_y) PTR_FIELD(lnr_rows) PTR_FIELD(lnr_gamma) PTR_FIELD(lnr_beta) PTR_FIELD(stats_out)
        PTR_FIELD(rows_out) PTR_FIELD(pool_part) PTR_FIELD(a_scale) PTR_FIELD(post_ln_w) PTR_FIELD(post_ln_b) PTR_FIELD(post_ln_out_half)
#undef PTR_FIELD
        if (key == "half_scale") { a.half_scale = (float)atof(tok.c_str() + eq + 1); continue; }
        if (key == "splitk_ws") { splitk_n = v; continue; }
        if (key == "cu") { n_cu = (int)v; continue; }
        if (key == "GEMM_VARIANT") { k.variant_set = true; k.variant = (int)v; continue; }
        if (key == "GEMM_SKINNY") { k.skinny = v != 0; continue; }
        if (key == "GEMM_GENERIC") { k.generic = v != 0; continue; }
        if (key == "GEMM_GRID") { k.grid = (int)v; continue; }
        if (key == "GEMM_TILE_ORDER") { k.tile_order = (int)v; continue; }
        if (key == "GEMM_NT") { k.nt = (int)v; continue; }
        if (key == "GEMM_256_MIN_TILES") { k.min_tiles = (int)v; continue; }
        if (key == "POST_LN") { k.post_ln = v != 0; continue; }
        if (key == "DEBUG_LDS_PAD") { k.lds_pad = (int)v; continue; }
        printf("?? %s\n", tok.c_str());
        return;
    }
    if (!a.lda) a.lda = a.K;
    if (!a.ldw) a.ldw = a.K;
    if (!a.ldh) a.ldh = a.N;
    if (!a.ldo) a.ldo = a.N;
    if (!a.ldraw) a.ldraw = a.N;
    if (!a.ldr) a.ldr = a.N;
    if (!a.ldrh) a.ldrh = a.N;
    if (!a.ldy) a.ldy = a.N;
    if (splitk_n >= 0) { a.splitk_ws = g_buf; a.splitk_bytes = sizeof(float) * (size_t)splitk_n * a.M * a.N; }
    if (ask) {      // the callers' questions, as gemm.hip's queries put them to the rule functions
        printf("streams=%d streaming_takes=%d post_ln_ok=%d skinny_takes=%d\n", (int)avx::gemm_rule_streams(a.M, a.N, k), (int)avx::gemm_rule_streaming_takes(a),
               (int)avx::gemm_rule_post_ln_ok(a, k), (int)avx::gemm_rule_skinny_takes(a.K, a.N, k));
        return;
    }
    g_err[0] = 0;
    avx::GemmPlan p;
    p.rc = avx::gemm_validate(a);
    if (p.rc == avx::PLAN_OK) p = avx::plan_gemm(a, n_cu, k);
    if (p.rc != avx::PLAN_OK) { printf("refused(%d): %s\n", p.rc, g_err); return; }
    switch (p.family) {
    case avx::GEMM_SKINNY: printf("skinny<NT=%d,KS=%d,SCALE=%d,RAW=%d> grid=%u", p.sk_nt, p.sk_ks, (int)p.sk_scale, (int)p.sk_raw, p.grid_x); break;
    case avx::GEMM_STREAM: printf("stream<%d,%d,%d> grid=%u", p.epi, p.ln, p.act, p.grid_x); break;
    case avx::GEMM_TILE128_REG: printf("tile128_reg grid=%u", p.grid_x); break;
    case avx::GEMM_TILE128_DMA: printf("tile128_dma grid=%ux%u S=%d", p.grid_x, p.grid_y, p.S); break;
    default: printf("no family"); break;
    }
    printf(" block=%d lds=%zu variant=%d gelu=%d", p.block, p.lds, p.args.variant, p.args.gelu);
    if (p.family == avx::GEMM_STREAM) printf(" nt=%d tile_order=%d", p.args.nt, p.args.tile_order);
    if (p.fold_lnr) printf(" fold_lnr");
    if (p.after == avx::GEMM_AFTER_SPLITK) printf(" then=splitk_epilogue[%u]", p.after_grid);
    if (p.after == avx::GEMM_AFTER_SPLITK_LN) printf(" then=splitk_ln_epilogue[%u]", p.after_grid);
    if (p.rows_out) printf(" then=ln_rowstats rows_out_arg=%d", p.args.rows_out != nullptr);
    printf("\n");
}

static void att_line(std::istringstream& in) {
    int T = 0, B = 0, H = 0, n_cu = 256;
    bool bias = false;
    avx::AttKnobs k;
    std::string tok;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        const std::string key = tok.substr(0, eq);
        const int v = eq == std::string::npos ? 0 : atoi(tok.c_str() + eq + 1);
        if (key == "T") T = v;
        else if (key == "B") B = v;
        else if (key == "H") H = v;
        else if (key == "cu") n_cu = v;
        else if (key == "bias") bias = true;
        else if (key == "ATT_VARIANT") k.variant = v;
        else if (key == "ATT_GRID") k.grid = v;
        else if (key == "ATT_TAIL_ROWS") k.tail_rows = v;
        else if (key == "ATT_NO_TAIL") k.no_tail = true;
        else if (key == "ATT_NO_XT") k.no_xt = true;
        else { printf("?? %s\n", tok.c_str()); return; }
    }
    g_err[0] = 0;
    const avx::AttPlan p = avx::plan_attention(T, B, H, bias, n_cu, k);
    if (p.rc != 0) { printf("refused(%d): %s\n", p.rc, g_err); return; }
    if (p.kernel == avx::ATT_KERNEL1) printf("attention_kernel");
    else if (p.kernel == avx::ATT_KERNEL2) printf("attention2<LONG=%d,BIAS=%d,XT=%d>", (int)p.k_long, (int)p.k_bias, (int)p.k_xt);
    else printf("attention3<BIAS=%d,XT=%d>", (int)p.k_bias, (int)p.k_xt);
    printf(" variant=%d grid=%u block=%d lds=%d per_block=%d nqb_main=%d", p.variant, p.grid, p.block, p.lds, p.per_block, p.nqb_main);
    if (p.use_tail) printf(" tail<RW=%d> rows=%d grid=%u lds=%zu", p.tail_rw, p.tail_rows, p.tail_grid, p.tail_lds);
    printf("\n");
}

int main() {
    char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "gemm") gemm_line(in, false);
        else if (kind == "ask") gemm_line(in, true);
        else if (kind == "att") att_line(in);
        else printf("?? %s\n", kind.c_str());
    }
    return 0;
}
