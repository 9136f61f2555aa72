"""Which kernel a product or an attention call gets, checked without a GPU: tests/dispatch/plan_dump.cpp -- its own main, the planner
headers (avex_amd/csrc/gemm_plan.h, attention_plan.h) and nothing else -- is built with the host C++ compiler and prints the plan of
every line it is given.  The expectations below were derived by hand from the launcher the planners replaced (gemm.hip launch<T>() /
avx::gemm(), attention.hip launch<T>() before the planners existed); each carries its derivation.  256 CUs, no knob set unless the line
sets one.  With AVEX_DISPATCH_SANITIZE=1 the program is built with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dispatch", "plan_dump.cpp")

BIG = "M=126976"      # 256 clips of 496 tokens
S5 = "block=512 lds=163840"      # the streaming kernel: 512 threads, two 64 KiB stages + 32 KiB of epilogue scratch
T128 = "block=256 lds=65536"     # the 128-tile kernels: two stages of two 16 KiB operand tiles
FOLD = "lnr_y lnr_rows lnr_gamma lnr_beta lnr_prefolded=1"

GEMM = [
    # QKV of a full batch: variant 0, K = 768 is no skinny width; 496 x 9 = 4464 tiles of 256^2 >= 128 -> streaming; more tiles than CUs ->
    # grid (256 / 8) * 8; half output + bias only -> fast epilogue EPI 1, no LayerNorm, no activation; N > 768 or not, NT mode 1 -> nt = 1
    (f"gemm {BIG} N=2304 K=768 out_half bias", f"stream<1,0,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    # ... reading raw rows through folded weights: LN bit 0
    (f"gemm {BIG} N=2304 K=768 out_half bias ln_rows ln_s", f"stream<1,1,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    # fc1: gelu 1 with a half output only becomes activation code 6 before anything else; the fast epilogue takes it as ACT 1
    (f"gemm {BIG} N=3072 K=768 out_half bias gelu=1", f"stream<1,0,1> grid=256 {S5} variant=0 gelu=6 nt=1 tile_order=0"),
    # ... but keeps the degree-6 form (code 1) when an fp32 output reads it too: generic epilogue (out_f32), no ACT template argument
    (f"gemm {BIG} N=3072 K=768 out_half out_f32 bias gelu=1", f"stream<0,0,0> grid=256 {S5} variant=0 gelu=1 nt=1 tile_order=0"),
    # out_proj under the fold: stats_out pins the streaming kernel; half residual -> EPI 2, LN bit 1 (statistics); rows_out is taken off the
    # kernel's arguments and ln_rowstats follows
    (f"gemm {BIG} N=768 K=768 out_half bias resid_half stats_out rows_out", f"stream<2,2,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0 then=ln_rowstats rows_out_arg=0"),
    # ... from the second layer on the residual is LayerNorm(raw y2) on the fly: LN bits 0 and 1
    (f"gemm {BIG} N=768 K=768 out_half bias {FOLD} stats_out", f"stream<2,3,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    # fc2 of the last layer under the fold: no statistics
    (f"gemm {BIG} N=768 K=3072 out_half bias {FOLD}", f"stream<2,1,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    # a caller's unfolded vectors: the same kernel, folded per launch by execute()
    (f"gemm {BIG} N=768 K=3072 out_half bias lnr_y lnr_rows lnr_gamma lnr_beta", f"stream<2,1,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0 fold_lnr"),
    # pooled taps: pool_part makes the output not "plain" -> generic epilogue, LN = pool_mode + 1
    (f"gemm {BIG} N=768 K=3072 out_half bias resid_half pool_part pool_T=496 pool_mode=0", f"stream<0,1,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    (f"gemm {BIG} N=768 K=3072 out_half bias resid_half pool_part pool_T=496 pool_mode=1", f"stream<0,2,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    (f"gemm {BIG} N=768 K=3072 out_half bias resid_half pool_part pool_T=496 pool_mode=2", f"stream<0,3,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    # one clip's fc2: 496 rows < 1024 -> 128-tile LDS-DMA, 4 x 6 = 24 tiles; workspace lent and K >= 1024 -> S = 8 (24 x 8 = 192 <= 2 x 256
    # workgroups, 3072 % 512 == 0, 384 >= 128 per split, 8 M N floats fit); epilogue over M N / 4 = 95 232 threads = 372 blocks
    ("gemm M=496 N=768 K=3072 out_half bias resid_half splitk_ws=8", f"tile128_dma grid=24x8 S=8 {T128} variant=0 gelu=0 then=splitk_epilogue[372]"),
    # ... with LayerNorm in the epilogue: one wave per row, four rows per block
    ("gemm M=496 N=768 K=3072 out_half bias resid_half splitk_ws=8 post_ln_w post_ln_b post_ln_out_half", f"tile128_dma grid=24x8 S=8 {T128} variant=0 gelu=0 then=splitk_ln_epilogue[124]"),
    # ... which works on whole rows of the workspace whatever K: out_proj (K = 768 < 1024) splits too, 768 = 4 x 192 (8 x 64 does not divide it)
    ("gemm M=496 N=768 K=768 out_half bias resid_half splitk_ws=8 post_ln_w post_ln_b post_ln_out_half", f"tile128_dma grid=24x4 S=4 {T128} variant=0 gelu=0 then=splitk_ln_epilogue[124]"),
    # eight clips: 16 x 9 = 144 tiles >= 128 -> streaming, grid = tiles rounded up to 8
    ("gemm M=3968 N=2304 K=768 out_half bias", f"stream<1,0,0> grid=144 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    # ... 16 x 3 = 48 tiles < 128 -> 128-tile, 31 x 6 tiles, no workspace -> one split, no epilogue kernel
    ("gemm M=3968 N=768 K=3072 out_half bias", f"tile128_dma grid=186x1 S=1 {T128} variant=0 gelu=0"),
    # pinned (batch-invariant handles): 2 x 3 tiles -> the smallest grid, 8
    ("gemm M=496 N=768 K=768 out_half bias variant=5", f"stream<1,0,0> grid=8 {S5} variant=5 gelu=0 nt=1 tile_order=0"),
    # variant 8: another name of variant 5
    ("gemm M=496 N=768 K=768 out_half bias variant=8", f"stream<1,0,0> grid=8 {S5} variant=5 gelu=0 nt=1 tile_order=0"),
    # ... and a pinned product the streaming kernel cannot take (N % 256) goes to the 128-tile kernel
    ("gemm M=496 N=640 K=768 out_half bias variant=5", f"tile128_dma grid=20x1 S=1 {T128} variant=5 gelu=0"),
    # EfficientNet's early 1 x 1 convolution: >= 32 768 rows, K % 64 == 0, N % 128 == 0, half only -> skinny NT = 128 / 16, KS = 64 / 32; W takes
    # 16 KiB -> 8 workgroups per CU by LDS, capped at 4 -> 1024 workgroups (64 128 row blocks)
    ("gemm M=8208384 N=128 K=64 out_half bias gelu=2", "skinny<NT=8,KS=2,SCALE=0,RAW=0> grid=1024 block=256 lds=16384 variant=0 gelu=2"),
    # forced, a width only the skinny kernel has: 8 row blocks
    ("gemm M=1000 N=96 K=32 out_half bias variant=7", "skinny<NT=6,KS=1,SCALE=0,RAW=0> grid=8 block=256 lds=6144 variant=7 gelu=0"),
    # ... with the squeeze-excitation scale and the raw tap
    ("gemm M=1000 N=64 K=96 out_half out_raw bias variant=7 a_scale a_scale_rows=100 a_scale_ld=96", "skinny<NT=4,KS=3,SCALE=1,RAW=1> grid=8 block=256 lds=12288 variant=7 gelu=0"),
    # the register-staged form takes the scale too
    ("gemm M=1000 N=128 K=512 out_half bias variant=1 a_scale a_scale_rows=100 a_scale_ld=512", f"tile128_reg grid=8 {T128} variant=1 gelu=0"),
    # narrow output rows: the 128-tile kernels only, even where the product would stream
    (f"gemm {BIG} N=256 K=768 out_half bias n_store=192 ldh=192", f"tile128_dma grid=1984x1 S=1 {T128} variant=0 gelu=0"),
    # ---- refusals, exact texts ----
    ("gemm M=1000 N=100 K=64 out_half", "refused(-1): gemm: N=100 must be a multiple of 128 (64 columns: the skinny streaming kernel only, >= 32768 rows)"),
    ("gemm M=1000 N=128 K=40 out_half", "refused(-1): gemm: K=40 must be a multiple of 64 (of 32 with the skinny kernel, variant 7)"),
    (f"gemm {BIG} N=768 K=768 out_half bias pool_part pool_T=32", "refused(-1): gemm: pool_part needs clips of at least 64 rows (got 32) and pool_mode 0..2 (got 0)"),
    (f"gemm {BIG} N=768 K=768 out_half bias ln_rows ln_s variant=3", "refused(-1): gemm: folded LayerNorm is built for the 256-tile kernel only"),
    (f"gemm {BIG} N=768 K=768 out_half bias variant=5 a_scale a_scale_rows=496 a_scale_ld=768", "refused(-1): gemm: a_scale is built for the skinny kernel (variant 7) and the register-staged 128-tile kernel (variant 1)"),
    (f"gemm {BIG} N=768 K=768 out_half bias stats_out rows_out variant=7", "refused(-1): gemm: variant 7 (skinny) takes K in {32, 64, 96, 128, 160, 256}, N in {32, 64, 96, 128, 160, 256} with N K <= 32768, a half output (N=768 K=768)"),
    ("gemm M=1000 N=128 K=64 out_half out_raw bias variant=7", "refused(-1): gemm: the skinny kernel writes a raw tap only for N = 32 / 64 / 128 / 256 with a_scale (N=128)"),
    ("gemm M=496 N=1280 K=768 out_half bias splitk_ws=8 post_ln_w post_ln_b post_ln_out_half", "refused(-1): gemm: post_ln_* needs the 128-tile kernel's workspace path (N % 256 == 0, N <= 1024, no activation, splitk_ws >= M N floats)"),
    # ---- knobs ----
    # GEMM_VARIANT=3: the variant of every variant-0 product; 992 x 18 tiles of 128^2
    (f"gemm {BIG} N=2304 K=768 out_half bias GEMM_VARIANT=3", f"tile128_dma grid=17856x1 S=1 {T128} variant=0 gelu=0"),
    # ... and, set at all, it switches the automatic skinny choice off, as GEMM_SKINNY=0 does: N = 128 is no multiple of 256 -> 128-tile, 64 128 tiles
    ("gemm M=8208384 N=128 K=64 out_half bias gelu=2 GEMM_SKINNY=0", f"tile128_dma grid=64128x1 S=1 {T128} variant=0 gelu=2"),
    ("gemm M=8208384 N=128 K=64 out_half bias gelu=2 GEMM_VARIANT=0", f"tile128_dma grid=64128x1 S=1 {T128} variant=0 gelu=2"),
    # ... except for 64 columns, which no other kernel takes
    ("gemm M=8208384 N=64 K=64 out_half bias GEMM_SKINNY=0", "skinny<NT=4,KS=2,SCALE=0,RAW=0> grid=1024 block=256 lds=8192 variant=0 gelu=0"),
    (f"gemm {BIG} N=2304 K=768 out_half bias GEMM_GENERIC=1", f"stream<0,0,0> grid=256 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    # 4 x 3 = 12 tiles: below the default threshold of 128 (128-tile, 8 x 6 tiles), above a threshold of 0 (grid 16)
    ("gemm M=1024 N=768 K=768 out_half bias", f"tile128_dma grid=48x1 S=1 {T128} variant=0 gelu=0"),
    ("gemm M=1024 N=768 K=768 out_half bias GEMM_256_MIN_TILES=0", f"stream<1,0,0> grid=16 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
    # GEMM_GRID rounds down to a multiple of 8; GEMM_TILE_ORDER and GEMM_NT reach the kernel's arguments (NT 5: hints only beyond 768 columns)
    (f"gemm {BIG} N=768 K=768 out_half bias GEMM_GRID=20 GEMM_TILE_ORDER=1 GEMM_NT=5", f"stream<1,0,0> grid=16 {S5} variant=0 gelu=0 nt=0 tile_order=1"),
    # POST_LN=0 makes the query say no; a caller that sets post_ln_* all the same is refused
    ("gemm M=496 N=768 K=3072 out_half bias splitk_ws=8 post_ln_w post_ln_b post_ln_out_half POST_LN=0", "refused(-1): gemm: post_ln_* needs the 128-tile kernel's workspace path (N % 256 == 0, N <= 1024, no activation, splitk_ws >= M N floats)"),
    ("gemm M=496 N=768 K=768 out_half bias DEBUG_LDS_PAD=64", "tile128_dma grid=24x1 S=1 block=256 lds=65600 variant=0 gelu=0"),
    # fewer CUs: the grid follows
    (f"gemm {BIG} N=2304 K=768 out_half bias cu=100", f"stream<1,0,0> grid=96 {S5} variant=0 gelu=0 nt=1 tile_order=0"),
]

# The questions callers ask instead of restating the launcher's rules (avx::gemm_streams, gemm_streaming_takes, gemm_post_ln_ok, gemm_skinny_takes)
QUERIES = [
    # one clip's fc2 with the workspace lent: too few rows to stream, but a shape the streaming kernel could be pinned to; LayerNorm may ride
    ("ask M=496 N=768 K=3072 out_half resid_half splitk_ws=8", "streams=0 streaming_takes=1 post_ln_ok=1 skinny_takes=0"),
    ("ask M=496 N=768 K=3072 out_half resid_half splitk_ws=8 POST_LN=0", "streams=0 streaming_takes=1 post_ln_ok=0 skinny_takes=0"),
    # ... not with an activation, not without the workspace, not when the caller pinned variant 5, not beyond 1024 columns
    ("ask M=496 N=768 K=768 out_half splitk_ws=8 gelu=1", "streams=0 streaming_takes=1 post_ln_ok=0 skinny_takes=0"),
    ("ask M=496 N=768 K=768 out_half", "streams=0 streaming_takes=1 post_ln_ok=0 skinny_takes=0"),
    ("ask M=496 N=768 K=768 out_half splitk_ws=8 variant=5", "streams=0 streaming_takes=1 post_ln_ok=0 skinny_takes=0"),
    ("ask M=496 N=1280 K=768 out_half splitk_ws=8", "streams=0 streaming_takes=1 post_ln_ok=0 skinny_takes=0"),
    # nine clips: 18 x 3 = 54 tiles < 128 for out_proj, 18 x 9 = 162 for QKV; a product that streams takes no post-LayerNorm
    ("ask M=4464 N=768 K=768 out_half splitk_ws=2", "streams=0 streaming_takes=1 post_ln_ok=1 skinny_takes=0"),
    ("ask M=4464 N=2304 K=768 out_half", "streams=1 streaming_takes=1 post_ln_ok=0 skinny_takes=0"),
    ("ask M=4464 N=768 K=768 out_half splitk_ws=2 GEMM_256_MIN_TILES=0", "streams=1 streaming_takes=1 post_ln_ok=0 skinny_takes=0"),
    # what the streaming kernel cannot take: K < 128, N % 256, half rows that are not 16-byte aligned
    ("ask M=4464 N=768 K=64 out_half", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=0"),
    ("ask M=4464 N=640 K=768 out_half", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=0"),
    ("ask M=4464 N=768 K=768 out_half ldh=772", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=0"),
    ("ask M=4464 N=768 K=768 out_half resid_half ldrh=772", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=0"),
    # EfficientNet's layout questions: widths 32 / 64 / 96 / 128 / 160 / 256 with N K <= 32768, unless the kernel is off or any variant is forced
    ("ask M=1 N=96 K=96", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=1"),
    ("ask M=1 N=160 K=160", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=1"),
    ("ask M=1 N=32 K=32", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=1"),
    ("ask M=1 N=256 K=128", "streams=0 streaming_takes=1 post_ln_ok=0 skinny_takes=1"),
    ("ask M=1 N=256 K=160", "streams=0 streaming_takes=1 post_ln_ok=0 skinny_takes=0"),
    ("ask M=1 N=192 K=64", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=0"),
    ("ask M=1 N=384 K=64", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=0"),
    ("ask M=1 N=96 K=96 GEMM_SKINNY=0", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=0"),
    ("ask M=1 N=96 K=96 GEMM_VARIANT=3", "streams=0 streaming_takes=0 post_ln_ok=0 skinny_takes=0"),
]

A3 = "block=512 lds=153376"       # attention3: two K+V halves of 64 KiB, four shifted bias rows, key mask, gate weights
ATTENTION = [
    # B H = 24 items, 256 workgroups allowed: one item each
    ("att T=496 B=2 H=12 bias", f"attention3<BIAS=1,XT=0> variant=3 grid=24 {A3} per_block=1 nqb_main=1"),
    ("att T=496 B=2 H=12", f"attention3<BIAS=0,XT=0> variant=3 grid=24 {A3} per_block=1 nqb_main=1"),
    # EAT: 513 = 512 + 1 -> the last row in the tail kernel (one row per wave; LDS 4 x (513 + 321) bytes), no bias table -> the first 512 query
    # rows in attention3's nine-tile form
    ("att T=513 B=2 H=12", "attention3<BIAS=0,XT=1> variant=2 grid=24 block=512 lds=152352 per_block=1 nqb_main=1 tail<RW=1> rows=1 grid=24 lds=3336"),
    # ... with a bias table: the long form of attention2, one query block + the tail
    ("att T=513 B=2 H=12 bias", "attention2<LONG=1,BIAS=1,XT=0> variant=2 grid=24 block=512 lds=158496 per_block=1 nqb_main=1 tail<RW=1> rows=1 grid=24 lds=3336"),
    # three rows beyond 512 are more than the tail takes (2): two query blocks; 515 % 256 = 3 keys ride as a ninth tile
    ("att T=515 B=2 H=12", "attention2<LONG=1,BIAS=0,XT=1> variant=2 grid=48 block=512 lds=150304 per_block=1 nqb_main=2"),
    # 600 % 256 = 88: no ninth tile
    ("att T=600 B=2 H=12", "attention2<LONG=1,BIAS=0,XT=0> variant=2 grid=48 block=512 lds=158496 per_block=1 nqb_main=2"),
    ("att T=1025 B=2 H=12 bias", "attention2<LONG=1,BIAS=1,XT=0> variant=2 grid=48 block=512 lds=158496 per_block=1 nqb_main=2 tail<RW=1> rows=1 grid=24 lds=5384"),
    ("att T=496 B=2 H=12 bias ATT_VARIANT=2", "attention2<LONG=0,BIAS=1,XT=0> variant=2 grid=24 block=512 lds=152352 per_block=1 nqb_main=1"),
    ("att T=496 B=2 H=12 ATT_VARIANT=2", "attention2<LONG=0,BIAS=0,XT=0> variant=2 grid=24 block=512 lds=152352 per_block=1 nqb_main=1"),
    ("att T=496 B=2 H=12 bias ATT_VARIANT=1", "attention_kernel variant=1 grid=24 block=1024 lds=150816 per_block=1 nqb_main=1"),
    # forcing variant 2 keeps EAT's main block in attention2 (ninth key tile)
    ("att T=513 B=2 H=12 ATT_VARIANT=2", "attention2<LONG=1,BIAS=0,XT=1> variant=2 grid=24 block=512 lds=150304 per_block=1 nqb_main=1 tail<RW=1> rows=1 grid=24 lds=3336"),
    # 18 tail rows: eight per wave (LDS 32 x (530 + 321) bytes), three groups per item
    ("att T=530 B=2 H=12 bias ATT_TAIL_ROWS=32", "attention2<LONG=1,BIAS=1,XT=0> variant=2 grid=24 block=512 lds=158496 per_block=1 nqb_main=1 tail<RW=8> rows=18 grid=72 lds=27232"),
    ("att T=513 B=2 H=12 ATT_NO_TAIL=1", "attention2<LONG=1,BIAS=0,XT=1> variant=2 grid=48 block=512 lds=150304 per_block=1 nqb_main=2"),
    ("att T=513 B=2 H=12 ATT_NO_XT=1", "attention2<LONG=1,BIAS=0,XT=0> variant=2 grid=24 block=512 lds=158496 per_block=1 nqb_main=1 tail<RW=1> rows=1 grid=24 lds=3336"),
    # three workgroups: eight consecutive items each
    ("att T=496 B=2 H=12 bias ATT_GRID=3", f"attention3<BIAS=1,XT=0> variant=3 grid=3 {A3} per_block=8 nqb_main=1"),
    ("att T=600 B=2 H=12 ATT_GRID=5", "attention2<LONG=1,BIAS=0,XT=0> variant=2 grid=5 block=512 lds=158496 per_block=10 nqb_main=2"),
]


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "a host C++ compiler (g++ / c++ / clang++) is needed to build tests/dispatch/plan_dump.cpp"
    exe = str(tmp_path_factory.mktemp("dispatch") / "plan_dump")
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra"]
    if os.environ.get("AVEX_DISPATCH_SANITIZE") == "1":
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([cxx] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=30)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr)
        out = p.stdout.splitlines()
        assert len(out) == len(lines), p.stdout
        return out
    return run


@pytest.mark.parametrize("table", [GEMM, QUERIES, ATTENTION], ids=["gemm", "queries", "attention"])
def test_plans(plan_dump, table):
    got = plan_dump([line for line, _ in table])
    wrong = [f"{line}\n    expected {want}\n    got      {g}" for (line, want), g in zip(table, got) if g != want]
    assert not wrong, "\n".join(wrong)
