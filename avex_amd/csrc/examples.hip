// Few-shot class scores from labelled example embeddings: for every query row and class the mean of the top_m largest similarities to
// the class's examples (nearest-example scoring), optionally minus the same value over the background examples.  The [queries, examples]
// similarity matrix is never stored.
//
// Layout: the bank is one [m, dpad] matrix of prepared rows (f32_prepare_rows) SORTED BY CLASS, background last, stable in the order the
// rows were added; row_id[column] is the row's number in that order.  A class is a column range; a SEGMENT is (class, 128-column tile):
// segments[s] = {class, first column, last column, tile}, in column order, tile_segments[t] .. tile_segments[t + 1] - 1 are the segments
// of tile t, class_segments[c] = {first, last} segment of class c (first > last: an empty class).  Class index n_classes is the background.
//
//   ex_prepare_kernel     query rows -> rows of dpad floats, the code of srch_prepare_kernel (f32_prepare_rows)
//   ex_tile_kernel        workgroup (column tile, 128-query tile): f32_tile_product as it is (queries are the A operand, as in
//                         srch_sim_kernel: the bits of a similarity are those a search returns), the tile written to LDS over the operand
//                         buffers (row stride EX_LDD, the padding of silhouette.hip), then thread (query row, parity) scans the columns of
//                         every second segment of the tile and keeps the top_m largest keys rank_key(similarity, row_id) (f32_tile.h: the
//                         search key with the insertion row) in a register list (depth a template parameter, insertion fully unrolled), NaN similarities skipped, unused
//                         entries 0.  The list goes to part[segment][batch row][top_m].
//   ex_reduce_kernel      thread (query, class): the lists of the class's consecutive segments merged into its top_m, their similarities
//                         added in fp32 in descending order from the largest, divided by float(count); NaN when there is none.  Launched
//                         for the background first (value per query into the workspace), then for the classes, which subtract it in
//                         margin mode and write scores[n][c] and nearest[n][c].
//   ex_class_mean_kernel  thread (output row, column): the fp32 sum over a range of bank rows in order, from 0.0f, divided by float(count).
//
// Keys are unique (a row appears once), so "the top_m largest keys of a class" is one set whatever the tiles and batches: a score is a
// function of the multiset of a class's similarities, and a similarity of its two rows.  No atomics of any kind; nothing here allocates
// or synchronises.
#include "f32_tile.h"

namespace {

constexpr int EX_MAX_TOP_M = 16;
constexpr int64_t EX_MAX_ROWS = 0x7fffffffll;                    // insertion rows are the low 32 key bits, inverted
constexpr int EX_MAX_CLASSES = 1 << 20, EX_MAX_BATCH = 1 << 22;  // what the second grid dimension of the two kernels holds
constexpr int EX_LDD = FT_BN + 4;                                // floats per row of the similarity tile in LDS: rows 528 B apart, so that
                                                                 // 16 threads reading 16 B of 16 consecutive rows hit 16 different bank quads
constexpr int EX_TILE_BYTES = FT_BM * EX_LDD * 4;                // 67 584 B >= FT_LDS_BYTES
constexpr int EX_LDS_BYTES = EX_TILE_BYTES + FT_BN * 4;          // + the inverted insertion rows of the tile's columns
static_assert(EX_TILE_BYTES >= FT_LDS_BYTES, "the similarity tile reuses the operand buffers; the row numbers lie behind them");

typedef unsigned long long ex_key_t;
typedef unsigned ex_u32x4 __attribute__((ext_vector_type(4)));

// A descending list of the DEPTH largest keys seen, in registers: every index below is a compile-time constant.
template <int DEPTH> static __device__ __forceinline__ void ex_clear(ex_key_t (&L)[DEPTH]) {
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) L[i] = 0ull;
}
template <int DEPTH> static __device__ __forceinline__ void ex_insert(ex_key_t (&L)[DEPTH], ex_key_t k) {
    if (k > L[DEPTH - 1]) {      // key 0 ("no key") never enters
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            const ex_key_t a = L[i];
            const bool up = k > a;
            L[i] = up ? k : a;
            k = up ? a : k;
        }
    }
}

__global__ __launch_bounds__(256) void ex_prepare_kernel(const float* __restrict__ x, int64_t ldx, int n, int d, int dpad, int normalise,
                                                         float* __restrict__ out) {
    f32_prepare_rows(x, ldx, n, d, dpad, normalise != 0, out);
}

struct TileArgs {
    const float* Q;                 // [nb, dpad] prepared queries
    const float* bank;              // [m, dpad]
    const int32_t* row_id;          // [m]
    const int32_t* segments;        // [n_segments][4]
    const int32_t* tile_segments;   // [n_tiles + 1]
    ex_key_t* part;                 // [n_segments][batch][top_m]
    int nb, m, dpad, n_segments, batch, top_m;
};

template <int DEPTH> __global__ __launch_bounds__(256) void ex_tile_kernel(TileArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tile = (float*)smem;
    unsigned* rid = (unsigned*)(smem + EX_TILE_BYTES);
    const int tid = threadIdx.x;
    const int t = blockIdx.x, c0 = t * FT_BN, q0 = blockIdx.y * FT_BM;
    if (tid < FT_BN) rid[tid] = c0 + tid < p.m ? rank_key_low((unsigned)p.row_id[c0 + tid]) : 0u;      // behind the operand buffers: free at once
    f32x16 acc[2][2];
    f32_tile_product(p.Q, p.nb, q0, p.bank, p.m, c0, p.dpad, acc);
    __syncthreads();      // every wave has read its last operand tile: the buffers become the similarity tile
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int lc = f32_tile_col(j);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) tile[f32_tile_row(i, r) * EX_LDD + lc] = acc[i][j][r];
    }
    __syncthreads();
    // the scanning role of this thread: query row qrow of the tile, the tile's segments of parity `par` (a wave has one parity: the loop
    // below is wave-uniform)
    const int qrow = tid & 127, par = tid >> 7;
    const bool mine = q0 + qrow < p.nb;
    int s0 = p.tile_segments[t], s1 = p.tile_segments[t + 1];
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > p.n_segments ? p.n_segments : s1;      // never a list outside part, whatever the caller's table holds
    const int top = p.m - c0 < FT_BN ? p.m - c0 : FT_BN;
    const float* trow = tile + qrow * EX_LDD;
    for (int s = s0 + par; s < s1; s += 2) {
        int lo = p.segments[4 * s + 1] - c0, hi = p.segments[4 * s + 2] - c0;      // inclusive
        lo = lo < 0 ? 0 : lo;
        hi = hi >= top ? top - 1 : hi;
        ex_key_t L[DEPTH];
        ex_clear(L);
        for (int q = lo >> 2; q <= (hi >> 2); ++q) {
            const f32x4 v = *(const f32x4*)(trow + 4 * q);
            const ex_u32x4 id = *(const ex_u32x4*)(rid + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = 4 * q + e;
                const float sim = v[e];
                const bool in = col >= lo && col <= hi && sim == sim;
                const ex_key_t key = rank_key_from_low(sim + 0.0f, id[e]);
                ex_insert(L, in ? key : 0ull);
            }
        }
        if (mine) {
            ex_key_t* o = p.part + ((int64_t)s * p.batch + (q0 + qrow)) * p.top_m;
#pragma unroll
            for (int i = 0; i < DEPTH; ++i)
                if (i < p.top_m) o[i] = L[i];
        }
    }
}

struct ReduceArgs {
    const ex_key_t* part;
    const int32_t* class_segments;      // [n_classes + 1][2]
    int n_segments, batch, nb, top_m;
    int c_lo, c_hi;                     // class indices [c_lo, c_hi)
    int qpb;                            // queries per workgroup: 256 / qpb classes share it
    int margin;
    const float* bg_in;                 // [batch]: subtracted in margin mode
    float* bg_out;                      // [batch]: the value goes here instead of scores (the background launch)
    float* scores;
    int64_t ld_scores;
    int32_t* nearest;
    int64_t ld_nearest;
};

template <int DEPTH> __global__ __launch_bounds__(256) void ex_reduce_kernel(ReduceArgs p) {
    const int tid = threadIdx.x;
    const int n = blockIdx.x * p.qpb + tid % p.qpb;
    const int c = p.c_lo + blockIdx.y * (256 / p.qpb) + tid / p.qpb;
    if (n >= p.nb || c >= p.c_hi) return;
    int s0 = p.class_segments[2 * c], s1 = p.class_segments[2 * c + 1];      // inclusive; s0 > s1: an empty class
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 >= p.n_segments ? p.n_segments - 1 : s1;
    ex_key_t L[DEPTH];
    ex_clear(L);
    for (int s = s0; s <= s1; ++s) {
        const ex_key_t* in = p.part + ((int64_t)s * p.batch + n) * p.top_m;
#pragma unroll
        for (int i = 0; i < DEPTH; ++i)
            if (i < p.top_m) ex_insert(L, in[i]);
    }
    float sum = 0.f;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < DEPTH; ++i)
        if (i < p.top_m && L[i] != 0ull) {      // descending, from the largest
            const float v = rank_key_value(L[i]);
            sum = cnt ? sum + v : v;
            ++cnt;
        }
    const float val = cnt ? sum / (float)cnt : __builtin_nanf("");
    if (p.bg_out) {
        p.bg_out[n] = val;
        return;
    }
    p.scores[(int64_t)n * p.ld_scores + c] = p.margin ? val - p.bg_in[n] : val;
    if (p.nearest) p.nearest[(int64_t)n * p.ld_nearest + c] = cnt ? (int32_t)rank_key_index(L[0]) : -1;
}

// out[k][col] = (sum over rows first[k] .. first[k] + count[k] - 1, in order, from 0.0f) / float(count[k]); zero beyond d
__global__ __launch_bounds__(256) void ex_class_mean_kernel(const float* __restrict__ rows, int64_t n_rows, int d, int dpad, const int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ count, float* __restrict__ out, int64_t ld_out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (col >= d) return;
    const int64_t r0 = first[k];
    const int cnt = count[k];
    float acc = 0.f;
    for (int64_t r = r0; r < r0 + cnt; ++r)
        if (r >= 0 && r < n_rows) acc = acc + rows[r * dpad + col];
    out[(int64_t)k * ld_out + col] = acc / (float)cnt;
}

struct Workspace {
    float* qn;
    ex_key_t* part;
    float* bg;
    size_t bytes;
};

static Workspace carve(void* ws, int batch, int n_segments, int top_m, int64_t dpad) {
    Workspace w;
    char* p = (char*)ws;
    w.qn = take<float>(p, (size_t)batch * (size_t)dpad);
    w.part = take<ex_key_t>(p, (size_t)n_segments * (size_t)batch * (size_t)top_m);
    w.bg = take<float>(p, (size_t)batch);
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

template <int DEPTH> static int launch(const avexhip_examples_args* a, const Workspace& w, int stages, hipStream_t s) {
    const int dp = (int)dpad_of(a->d);
    const int n_tiles = (int)((a->m + FT_BN - 1) / FT_BN);
    if (stages & 1) {
        TileArgs t;
        t.Q = w.qn;
        t.bank = a->bank;
        t.row_id = a->row_id;
        t.segments = a->segments;
        t.tile_segments = a->tile_segments;
        t.part = w.part;
        t.nb = a->n;
        t.m = (int)a->m;
        t.dpad = dp;
        t.n_segments = a->n_segments;
        t.batch = a->batch;
        t.top_m = a->top_m;
        AVX_ENSURE_LDS(ex_tile_kernel<DEPTH>, EX_LDS_BYTES);
        ex_tile_kernel<DEPTH><<<dim3(n_tiles, (a->n + FT_BM - 1) / FT_BM), dim3(256), EX_LDS_BYTES, s>>>(t);
        AVX_LAUNCH_CHECK();
    }
    if (stages & 2) {
        ReduceArgs r;
        r.part = w.part;
        r.class_segments = a->class_segments;
        r.n_segments = a->n_segments;
        r.batch = a->batch;
        r.nb = a->n;
        r.top_m = a->top_m;
        r.margin = a->mode == AVEXHIP_EXAMPLES_MARGIN;
        r.bg_in = w.bg;
        r.scores = a->scores;
        r.ld_scores = a->ld_scores;
        r.nearest = a->nearest;
        r.ld_nearest = a->ld_nearest;
        r.c_lo = 0;
        r.c_hi = a->n_classes;
        r.qpb = 16;
        r.bg_out = nullptr;
        if (r.margin) {      // the background value of every query first: class index n_classes
            ReduceArgs b = r;
            b.c_lo = a->n_classes;
            b.c_hi = a->n_classes + 1;
            b.qpb = 256;
            b.bg_out = w.bg;
            ex_reduce_kernel<DEPTH><<<dim3((a->n + 255) / 256, 1), dim3(256), 0, s>>>(b);
            AVX_LAUNCH_CHECK();
        }
        ex_reduce_kernel<DEPTH><<<dim3((a->n + 15) / 16, (a->n_classes + 15) / 16), dim3(256), 0, s>>>(r);
        AVX_LAUNCH_CHECK();
    }
    return AVEXHIP_OK;
}

}  // namespace

extern "C" int avexhip_examples_max_top_m(void) { return EX_MAX_TOP_M; }

extern "C" size_t avexhip_examples_workspace_bytes(int batch, int n_segments, int top_m, int dpad) {
    if (batch <= 0 || batch > EX_MAX_BATCH || n_segments <= 0 || top_m <= 0 || top_m > EX_MAX_TOP_M || dpad <= 0 || dpad % FT_BK != 0) return 0;
    return carve(nullptr, batch, n_segments, top_m, dpad).bytes;
}

extern "C" int avexhip_examples_score(const avexhip_examples_args* a, void* stream) {
    AVX_REQUIRE(a && a->bank && a->row_id && a->segments && a->tile_segments && a->class_segments && a->query && a->workspace && a->scores,
                "examples_score: null argument");
    AVX_REQUIRE(a->m >= 1 && a->m <= EX_MAX_ROWS && a->d >= 1 && a->n_classes >= 1 && a->n_classes <= EX_MAX_CLASSES,
                "examples_score: bad bank (m %lld [1, 2^31 - 1], d %d, n_classes %d [1, %d])", (long long)a->m, a->d, a->n_classes, EX_MAX_CLASSES);
    const int64_t n_tiles = (a->m + FT_BN - 1) / FT_BN;
    AVX_REQUIRE(a->n_segments >= n_tiles && a->n_segments <= n_tiles + a->n_classes, "examples_score: n_segments %d outside [%lld, %lld] for %lld rows and %d classes",
                a->n_segments, (long long)n_tiles, (long long)(n_tiles + a->n_classes), (long long)a->m, a->n_classes);
    AVX_REQUIRE(a->batch >= 1 && a->batch <= EX_MAX_BATCH && a->n >= 1 && a->n <= a->batch, "examples_score: bad batch (batch %d [1, %d], n %d)", a->batch,
                EX_MAX_BATCH, a->n);
    AVX_REQUIRE(a->top_m >= 1 && a->top_m <= EX_MAX_TOP_M, "examples_score: top_m %d outside [1, %d]", a->top_m, EX_MAX_TOP_M);
    AVX_REQUIRE(a->mode == AVEXHIP_EXAMPLES_SIMILARITY || a->mode == AVEXHIP_EXAMPLES_MARGIN, "examples_score: mode %d is neither 0 nor 1", a->mode);
    AVX_REQUIRE(a->normalise == 0 || a->normalise == 1, "examples_score: normalise %d is neither 0 nor 1", a->normalise);
    AVX_REQUIRE(a->ld_query >= a->d, "examples_score: ld_query %lld < d %d", (long long)a->ld_query, a->d);
    AVX_REQUIRE(a->ld_scores >= a->n_classes, "examples_score: ld_scores %lld < %d classes", (long long)a->ld_scores, a->n_classes);
    if (a->nearest) AVX_REQUIRE(a->ld_nearest >= a->n_classes, "examples_score: ld_nearest %lld < %d classes", (long long)a->ld_nearest, a->n_classes);
    const int stages = a->stages == 0 ? 3 : a->stages;
    AVX_REQUIRE(stages >= 1 && stages <= 3, "examples_score: stages %d outside 0 .. 3", a->stages);
    const Workspace w = carve(a->workspace, a->batch, a->n_segments, a->top_m, dpad_of(a->d));
    if (a->workspace_bytes < w.bytes) {
        avexhip_set_error("examples_score: workspace %zu B < %zu B", a->workspace_bytes, w.bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    if (stages & 1) {
        ex_prepare_kernel<<<dim3((a->n + 3) / 4), dim3(256), 0, s>>>(a->query, a->ld_query, a->n, a->d, (int)dpad_of(a->d), a->normalise, w.qn);
        AVX_LAUNCH_CHECK();
    }
    if (a->top_m == 1) return launch<1>(a, w, stages, s);
    if (a->top_m == 2) return launch<2>(a, w, stages, s);
    if (a->top_m <= 4) return launch<4>(a, w, stages, s);
    if (a->top_m <= 8) return launch<8>(a, w, stages, s);
    return launch<16>(a, w, stages, s);
}

extern "C" int avexhip_examples_class_mean(const float* rows_dev, int64_t n_rows, int d, const int32_t* first_dev, const int32_t* count_dev, int n_out,
                                           float* out_dev, int64_t ld_out, void* stream) {
    AVX_REQUIRE(rows_dev && first_dev && count_dev && out_dev, "examples_class_mean: null argument");
    AVX_REQUIRE(n_rows >= 1 && n_rows <= EX_MAX_ROWS && d >= 1, "examples_class_mean: bad shape (n_rows %lld, d %d)", (long long)n_rows, d);
    AVX_REQUIRE(n_out >= 1 && n_out <= 65535, "examples_class_mean: n_out %d outside [1, 65535]", n_out);
    AVX_REQUIRE(ld_out >= d, "examples_class_mean: ld_out %lld < d %d", (long long)ld_out, d);
    ex_class_mean_kernel<<<dim3((d + 255) / 256, n_out), dim3(256), 0, (hipStream_t)stream>>>(rows_dev, n_rows, d, (int)dpad_of(d), first_dev, count_dev, out_dev,
                                                                                              ld_out);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
