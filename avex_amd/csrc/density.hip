// Density clustering (DBSCAN) over embeddings that already live in HBM: which rows lie within eps of at least min_samples rows (core
// rows), the connected components of the core rows, and the border rows that hang on them.  O(N^2 D) thresholded distances on the fp32
// MFMA tile of f32_tile.h per pass, O(N) integers of working memory; the N x N matrix is never written.
//
// The rows come in blocks (the chunks of an EmbeddingIndex, or pieces of them): every tile launcher takes a row block and a column block
// of prepared rows with the global number of their first row, and the caller walks the block pairs.  Per-row state lives in the workspace
// under global row numbers.
//
//   dens_diag_kernel      ||row||^2 as the DIAGONAL of the tile product (sil_diag_kernel's argument: bit-identical rows are at distance
//                         exactly 0).  A row whose squared norm is not a finite number is OUTSIDE the graph: it holds a NaN or an Inf.
//   dens_walk_kernel      workgroup (column segment, 128-row tile): for each 128-column tile of its segment the product, then
//                             cosine      d = min(max(1 - s, 0), 2)                            sil_dist_kernel's expressions
//                             euclidean   d = sqrt(max((nx + ny) - 2 s, 0))
//                         and the predicate  both rows inside the graph  &&  (d <= eps || same row).  Every lane keeps one running integer
//                         per accumulator register over ALL the column tiles of the segment -- COUNT: the number of true predicates;
//                         HOOK: the minimum of label[column] over the true ones whose column is a core row -- and only after the last tile
//                         are they reduced over the 32 lanes that hold one row (shuffles), over the two waves that share the rows (LDS),
//                         and sent out with ONE integer atomic per (row, workgroup): atomicAdd into n_neighbors[row], or atomicMin into
//                         next[row] and, when the row is core, into next[label[row]] (the hook of its root).
//   dens_core_kernel      core = inside && n_neighbors >= min_samples; label = own row for a core row, NONE otherwise; the outside rows
//   dens_begin_kernel     next = label                                       (start of a round)
//   dens_apply_kernel     core rows: label = min(label, next), the changed flag
//   dens_compress_kernel  pointer jumping to the fixed point: every core row follows label[label[..]] down to the row that points at
//                         itself and takes it.  Labels only decrease and a label is never larger than its row, so the chains end.
//   prefix_count          (prefix_count.h, shared with regions.hip) roots (label == own row) counted per 1 024 rows, an exclusive prefix
//                         over the blocks, then the rank inside the block: cluster numbers in the order of the lowest core row, by counting
//   dens_labels_kernel    core row: the number of its root; other row: the number of next[row], the smallest root among its core
//                         neighbours as the last (unchanged) round left it, or -1
//   dens_sizes_kernel     per cluster its size (atomicAdd) and the key (n_neighbors << 32) | (0xFFFFFFFF - row) of its best core row
//                         (64-bit atomicMax), the lanes of a wave that share a cluster combined first
//   dens_exemplar_kernel  key -> row
//
// Symmetry.  s(i, j) and s(j, i) are the same bits: f32_tile_product gives both operands the same k assignment and adds the terms in the
// same order, so which of the two rows is A does not matter.  The neighbour relation is therefore exactly symmetric, and "row i counts
// j" and "row j counts i" are one fact.
// Determinism.  Every atomic is an integer add, min or max on global memory: order-free.  Counts, labels and keys are integers, so the
// result does not depend on the segments, the blocks, or the run.  No float atomics.
// Limits: n <= 2^31 - 1 rows, dpad % 32 == 0, a block of at most 2^22 rows.
#include "block_prims.h"
#include "f32_tile.h"
#include "prefix_count.h"

namespace {

constexpr int DN_NONE = 0x7fffffff;                              // "no label": not a core row / no core neighbour
constexpr int64_t DN_MAX_N = 0x7fffffffll;
constexpr int DN_MAX_BLOCK = 1 << 22;                            // rows of one block: 32 768 row tiles, the second grid dimension
constexpr int DN_LDS_BYTES = FT_LDS_BYTES + 2 * FT_BM * 4;       // the operand buffers, and behind them one integer per (column wave, row)
constexpr float DN_FLT_MAX = 3.4028234663852886e38f;

struct Workspace {
    float* nrm;                  // [n] squared norm from the diagonal; not finite: the row is outside the graph
    int32_t *count, *label, *next, *cid;      // [n] each
    unsigned long long* keys;    // [n] exemplar keys, by cluster
    int32_t* block;              // [prefix_count_blocks(n)] roots per block, then their exclusive prefix
    int32_t* flags;              // [0] rows outside the graph, [1] clusters
    size_t bytes;
};

static Workspace carve(void* ws, int64_t n) {
    Workspace w;
    char* p = (char*)ws;
    w.nrm = take<float>(p, (size_t)n);
    w.count = take<int32_t>(p, (size_t)n);
    w.label = take<int32_t>(p, (size_t)n);
    w.next = take<int32_t>(p, (size_t)n);
    w.cid = take<int32_t>(p, (size_t)n);
    w.keys = take<unsigned long long>(p, (size_t)n);
    w.block = take<int32_t>(p, (size_t)prefix_count_blocks(n));
    w.flags = take<int32_t>(p, 4);
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

static __device__ __forceinline__ bool dn_finite(float v) { return __builtin_fabsf(v) <= DN_FLT_MAX; }      // false for a NaN

__global__ __launch_bounds__(256) void dens_diag_kernel(const float* __restrict__ rows, int n_rows, int dpad, float* __restrict__ nrm) {
    const int r0 = blockIdx.x * FT_BM;
    f32x16 acc[2][2];
    f32_tile_product(rows, n_rows, r0, rows, n_rows, r0, dpad, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = f32_tile_col(j);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (f32_tile_row(i, r) == col && r0 + col < n_rows) nrm[r0 + col] = acc[i][j][r];
        }
}

struct WalkArgs {
    const float *rows, *cols;      // the two blocks of prepared rows
    int n_rows, n_cols;
    int64_t row0, col0;            // global number of their first rows
    int dpad, tiles_per_seg;
    float eps;
    int64_t n;
    const float* nrm;              // [n]
    const int32_t* label;          // [n] (HOOK)
    int32_t* out;                  // [n] n_neighbors (COUNT) or next (HOOK)
};

template <bool HOOK, bool EUCLID> __global__ __launch_bounds__(256) void dens_walk_kernel(WalkArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* red = (int*)(smem + FT_LDS_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wc = (tid >> 6) & 1;
    const int r0 = blockIdx.y * FT_BM;
    const int n_tiles = (p.n_cols + FT_BN - 1) / FT_BN;
    const int t0 = blockIdx.x * p.tiles_per_seg;
    const int t1 = t0 + p.tiles_per_seg < n_tiles ? t0 + p.tiles_per_seg : n_tiles;
    const float* rnrm = p.nrm + p.row0;
    const float* cnrm = p.nrm + p.col0;
    const int32_t* clabel = p.label + p.col0;
    // tile row - tile column of acc[i][j][r] is dlt + 32 i + (r & 3) + 8 (r >> 2) - 32 j (f32_tile_row / f32_tile_col): the part that
    // depends on the thread, in one register, so that "the same global row" is one compare with a constant
    const int dlt = f32_tile_row(0, 0) - f32_tile_col(0);
    float rn[2][16];
    unsigned rok = 0u;      // bit 16 i + r: that row of mine is a row of the block and inside the graph
    int av[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + f32_tile_row(i, r);
            const float v = row < p.n_rows ? rnrm[row] : __builtin_nanf("");
            rn[i][r] = v;
            rok |= dn_finite(v) ? 1u << (16 * i + r) : 0u;
            av[i][r] = HOOK ? DN_NONE : 0;
        }
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * FT_BN;
        const int64_t off = (p.col0 + c0) - (p.row0 + r0);      // tile row lr and tile column lc are the same global row iff lr - lc == off
        const int offd = off > -FT_BN && off < FT_BM ? (int)off - dlt : -(1 << 30);
        f32x16 acc[2][2];
        f32_tile_product(p.rows, p.n_rows, r0, p.cols, p.n_cols, c0, p.dpad, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = f32_tile_col(j);
            const bool inb = c0 + lc < p.n_cols;
            const float cn = inb ? cnrm[c0 + lc] : __builtin_nanf("");
            const bool cok = dn_finite(cn);
            int lab = DN_NONE;
            if (HOOK) lab = cok ? clabel[c0 + lc] : DN_NONE;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float g = acc[i][j][r];
                    float dv;
                    if (EUCLID) {
                        const float d2 = (rn[i][r] + cn) - 2.0f * g;
                        dv = __builtin_sqrtf(d2 > 0.f ? d2 : 0.f);      // the correctly rounded root: the threshold is compared with NumPy's bits
                    } else {
                        dv = 1.0f - g;
                        dv = dv < 0.f ? 0.f : (dv > 2.f ? 2.f : dv);
                    }
                    const bool pred = cok && ((rok >> (16 * i + r)) & 1u) && (dv <= p.eps || offd == 32 * i + (r & 3) + 8 * (r >> 2) - 32 * j);
                    if (HOOK) {
                        const int cand = pred ? lab : DN_NONE;
                        av[i][r] = cand < av[i][r] ? cand : av[i][r];
                    } else {
                        av[i][r] += pred ? 1 : 0;
                    }
                }
        }
        __syncthreads();      // every wave has read its last operand tile: the next product stages over the buffers
    }
    // over the 32 lanes of a half wave (the 32 columns of one row), then over the two waves that share the rows
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int v = av[i][r];
#pragma unroll
            for (int s = 16; s > 0; s >>= 1) {
                const int o = __shfl_xor(v, s);
                v = HOOK ? (o < v ? o : v) : v + o;
            }
            if ((lane & 31) == 0) red[wc * FT_BM + f32_tile_row(i, r)] = v;
        }
    __syncthreads();
    if (tid < FT_BM && r0 + tid < p.n_rows) {
        const int a = red[tid], b = red[FT_BM + tid];
        const int64_t g = p.row0 + r0 + tid;
        if (HOOK) {
            const int v = a < b ? a : b;
            if (v != DN_NONE) {
                const int mine = p.label[g];
                if (mine == DN_NONE) atomicMin(p.out + g, v);      // not core: receives, never gives
                else if (v < mine) {
                    atomicMin(p.out + g, v);
                    if (mine >= 0 && mine < p.n) atomicMin(p.out + mine, v);      // the root's hook
                }
            }
        } else if (a + b != 0) {
            atomicAdd(p.out + g, a + b);
        }
    }
}

// 256 rows per workgroup; no thread leaves before the block-wide count
__global__ __launch_bounds__(256) void dens_core_kernel(int64_t n, const float* __restrict__ nrm, int32_t* __restrict__ count, int min_samples,
                                                        int32_t* __restrict__ label, int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        bad = !dn_finite(nrm[i]);
        if (bad) count[i] = 0;
        label[i] = !bad && count[i] >= min_samples ? (int32_t)i : DN_NONE;
    }
    const int c = __syncthreads_count(bad);
    if (threadIdx.x == 0 && c) atomicAdd(flags, c);
}

__global__ __launch_bounds__(256) void dens_begin_kernel(int64_t n, const int32_t* __restrict__ label, int32_t* __restrict__ next) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) next[i] = label[i];
}

__global__ __launch_bounds__(256) void dens_apply_kernel(int64_t n, int32_t* __restrict__ label, const int32_t* __restrict__ next,
                                                         int32_t* __restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int ch = 0;
    if (i < n) {
        const int l = label[i], nx = next[i];
        if (l != DN_NONE && nx < l && nx >= 0) {
            label[i] = nx;
            ch = 1;
        }
    }
    if (__syncthreads_or(ch) && threadIdx.x == 0) *changed = 1;
}

// Other threads write label[k] = (an ancestor of k) meanwhile: whichever value a read sees lies on the same chain, and every step goes to a
// strictly smaller row.
__global__ __launch_bounds__(256) void dens_compress_kernel(int64_t n, int32_t* label) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = label[i];
    if (l == DN_NONE || l < 0 || l >= i) return;      // not core, or a root
    int r = l;
    for (;;) {
        const int q = __atomic_load_n(label + r, __ATOMIC_RELAXED);
        if (q < 0 || q >= r) break;
        r = q;
    }
    if (r != l) __atomic_store_n(label + i, r, __ATOMIC_RELAXED);
}

// the cluster numbers by counting (prefix_count.h): a root counts 1, takes its rank; every other row takes -1
struct DnIsRoot {
    const int32_t* label;
    __device__ __forceinline__ bool operator()(int64_t i) const { return label[i] == i; }
};
struct DnStoreCid {
    int32_t* cid;
    __device__ __forceinline__ void operator()(int64_t i, int rank, bool root) const { cid[i] = root ? rank : -1; }
};

__global__ __launch_bounds__(256) void dens_labels_kernel(int64_t n, const int32_t* __restrict__ label, const int32_t* __restrict__ next,
                                                          const int32_t* __restrict__ cid, const int32_t* __restrict__ count, const int32_t* __restrict__ flags,
                                                          int32_t* __restrict__ labels_out, uint8_t* __restrict__ core_out, int32_t* __restrict__ nn_out,
                                                          int32_t* __restrict__ summary) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        summary[0] = flags[1];
        summary[1] = flags[0];
    }
    if (i >= n) return;
    const int l = label[i];
    const int src = l != DN_NONE ? l : next[i];
    labels_out[i] = src >= 0 && src < n ? cid[src] : -1;
    core_out[i] = l != DN_NONE ? 1 : 0;
    nn_out[i] = count[i];
}

// No thread leaves before the wave's loop: its shuffles and ballots take all 64 lanes.
__global__ __launch_bounds__(256) void dens_sizes_kernel(int64_t n, const int32_t* __restrict__ labels, const int32_t* __restrict__ label,
                                                         const int32_t* __restrict__ count, int n_clusters, int32_t* __restrict__ sizes,
                                                         unsigned long long* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int c = -1;
    unsigned long long key = 0ull;
    if (i < n) {
        c = labels[i];
        c = c < n_clusters ? c : -1;
        if (c >= 0 && label[i] != DN_NONE) key = rank_key((unsigned)count[i], (unsigned)i);
    }
    unsigned long long todo = __ballot(c >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(c, leader);
        const bool same = c == lc;
        const unsigned long long mask = __ballot(same);
        const unsigned long long k = wave_reduce(same ? key : 0ull, BlockMax());
        if (lane == leader) {
            atomicAdd(sizes + lc, __popcll(mask));
            if (k) atomicMax(keys + lc, k);
        }
        todo &= ~mask;
    }
}

__global__ __launch_bounds__(256) void dens_exemplar_kernel(int n_clusters, const unsigned long long* __restrict__ keys, int32_t* __restrict__ exemplar) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_clusters) return;
    const unsigned long long k = keys[c];
    exemplar[c] = k ? (int32_t)rank_key_index(k) : -1;
}

static int check_args(const avexhip_density_args* a, const char* what, Workspace* w) {
    AVX_REQUIRE(a && a->workspace, "%s: null argument", what);
    AVX_REQUIRE(a->n >= 1 && a->n <= DN_MAX_N, "%s: n %lld outside [1, 2^31 - 1]", what, (long long)a->n);
    AVX_REQUIRE(a->dpad >= FT_BK && a->dpad % FT_BK == 0, "%s: dpad %d is not a positive multiple of %d", what, a->dpad, FT_BK);
    AVX_REQUIRE(a->metric == AVEXHIP_DENSITY_EUCLIDEAN || a->metric == AVEXHIP_DENSITY_COSINE, "%s: metric %d", what, a->metric);
    *w = carve(a->workspace, a->n);
    if (a->workspace_bytes < w->bytes) {
        avexhip_set_error("%s: workspace %zu B < %zu B", what, a->workspace_bytes, w->bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    return AVEXHIP_OK;
}

static int check_rows(const avexhip_density_args* a, const char* what) {
    AVX_REQUIRE(a->rows && a->n_rows >= 1 && a->n_rows <= DN_MAX_BLOCK && a->row0 >= 0 && a->row0 + a->n_rows <= a->n,
                "%s: row block [%lld, +%d) outside [0, %lld) or above %d rows", what, (long long)a->row0, a->n_rows, (long long)a->n, DN_MAX_BLOCK);
    return AVEXHIP_OK;
}

static int check_cols(const avexhip_density_args* a, const char* what) {
    AVX_REQUIRE(a->cols && a->n_cols >= 1 && a->n_cols <= DN_MAX_BLOCK && a->col0 >= 0 && a->col0 + a->n_cols <= a->n,
                "%s: column block [%lld, +%d) outside [0, %lld) or above %d rows", what, (long long)a->col0, a->n_cols, (long long)a->n, DN_MAX_BLOCK);
    AVX_REQUIRE(a->eps >= 0.f && a->eps <= DN_FLT_MAX, "%s: eps %g is not a finite number >= 0", what, (double)a->eps);
    return AVEXHIP_OK;
}

template <bool HOOK> static int walk(const avexhip_density_args* a, const Workspace& w, hipStream_t s) {
    WalkArgs p;
    p.rows = a->rows;
    p.cols = a->cols;
    p.n_rows = a->n_rows;
    p.n_cols = a->n_cols;
    p.row0 = a->row0;
    p.col0 = a->col0;
    p.dpad = a->dpad;
    p.eps = a->eps;
    p.n = a->n;
    p.nrm = w.nrm;
    p.label = w.label;
    p.out = HOOK ? w.next : w.count;
    const int row_tiles = (a->n_rows + FT_BM - 1) / FT_BM, n_tiles = (a->n_cols + FT_BN - 1) / FT_BN;
    int segs = 2048 / row_tiles;      // enough workgroups to fill the chip several times; the result does not depend on this
    segs = segs < 1 ? 1 : (segs > n_tiles ? n_tiles : segs);
    p.tiles_per_seg = (n_tiles + segs - 1) / segs;
    const dim3 grid((n_tiles + p.tiles_per_seg - 1) / p.tiles_per_seg, row_tiles);
    if (a->metric == AVEXHIP_DENSITY_EUCLIDEAN) {
        AVX_ENSURE_LDS((dens_walk_kernel<HOOK, true>), DN_LDS_BYTES);
        dens_walk_kernel<HOOK, true><<<grid, dim3(256), DN_LDS_BYTES, s>>>(p);
    } else {
        AVX_ENSURE_LDS((dens_walk_kernel<HOOK, false>), DN_LDS_BYTES);
        dens_walk_kernel<HOOK, false><<<grid, dim3(256), DN_LDS_BYTES, s>>>(p);
    }
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

static unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" size_t avexhip_density_workspace_bytes(int64_t n) {
    if (n <= 0 || n > DN_MAX_N) return 0;
    return carve(nullptr, n).bytes;
}

extern "C" int avexhip_density_max_block(void) { return DN_MAX_BLOCK; }

extern "C" int avexhip_density_begin(const avexhip_density_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_begin", &w));
    hipStream_t s = (hipStream_t)stream;
    AVX_HIP_CHECK(hipMemsetAsync(w.count, 0, (size_t)a->n * 4, s));
    AVX_HIP_CHECK(hipMemsetAsync(w.flags, 0, 16, s));
    return AVEXHIP_OK;
}

extern "C" int avexhip_density_norms(const avexhip_density_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_norms", &w));
    AVXH_TRY(check_rows(a, "density_norms"));
    AVX_ENSURE_LDS(dens_diag_kernel, FT_LDS_BYTES);
    dens_diag_kernel<<<dim3((a->n_rows + FT_BM - 1) / FT_BM), dim3(256), FT_LDS_BYTES, (hipStream_t)stream>>>(a->rows, a->n_rows, a->dpad, w.nrm + a->row0);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_density_count(const avexhip_density_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_count", &w));
    AVXH_TRY(check_rows(a, "density_count"));
    AVXH_TRY(check_cols(a, "density_count"));
    return walk<false>(a, w, (hipStream_t)stream);
}

extern "C" int avexhip_density_core(const avexhip_density_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_core", &w));
    AVX_REQUIRE(a->min_samples >= 1, "density_core: min_samples %d < 1", a->min_samples);
    dens_core_kernel<<<dim3(blocks256(a->n)), dim3(256), 0, (hipStream_t)stream>>>(a->n, w.nrm, w.count, a->min_samples, w.label, w.flags);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_density_round_begin(const avexhip_density_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_round_begin", &w));
    dens_begin_kernel<<<dim3(blocks256(a->n)), dim3(256), 0, (hipStream_t)stream>>>(a->n, w.label, w.next);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_density_hook(const avexhip_density_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_hook", &w));
    AVXH_TRY(check_rows(a, "density_hook"));
    AVXH_TRY(check_cols(a, "density_hook"));
    return walk<true>(a, w, (hipStream_t)stream);
}

extern "C" int avexhip_density_round_end(const avexhip_density_args* a, int32_t* changed_out_dev, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_round_end", &w));
    AVX_REQUIRE(changed_out_dev, "density_round_end: null output");
    hipStream_t s = (hipStream_t)stream;
    AVX_HIP_CHECK(hipMemsetAsync(changed_out_dev, 0, 4, s));
    dens_apply_kernel<<<dim3(blocks256(a->n)), dim3(256), 0, s>>>(a->n, w.label, w.next, changed_out_dev);
    AVX_LAUNCH_CHECK();
    dens_compress_kernel<<<dim3(blocks256(a->n)), dim3(256), 0, s>>>(a->n, w.label);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_density_labels(const avexhip_density_args* a, int32_t* labels_out_dev, uint8_t* core_out_dev, int32_t* n_neighbors_out_dev,
                                      int32_t* summary_out_dev, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_labels", &w));
    AVX_REQUIRE(labels_out_dev && core_out_dev && n_neighbors_out_dev && summary_out_dev, "density_labels: null output");
    hipStream_t s = (hipStream_t)stream;
    AVXH_TRY(prefix_count<int32_t>(a->n, PrefixHostN{a->n}, DnIsRoot{w.label}, w.block, w.flags + 1, DnStoreCid{w.cid}, s));
    dens_labels_kernel<<<dim3(blocks256(a->n)), dim3(256), 0, s>>>(a->n, w.label, w.next, w.cid, w.count, w.flags, labels_out_dev, core_out_dev,
                                                                  n_neighbors_out_dev, summary_out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_density_summary(const avexhip_density_args* a, const int32_t* labels_dev, int n_clusters, int32_t* sizes_out_dev,
                                       int32_t* exemplar_out_dev, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "density_summary", &w));
    AVX_REQUIRE(labels_dev && sizes_out_dev && exemplar_out_dev, "density_summary: null argument");
    AVX_REQUIRE(n_clusters >= 1 && n_clusters <= a->n, "density_summary: n_clusters %d outside [1, n]", n_clusters);
    hipStream_t s = (hipStream_t)stream;
    AVX_HIP_CHECK(hipMemsetAsync(sizes_out_dev, 0, (size_t)n_clusters * 4, s));
    AVX_HIP_CHECK(hipMemsetAsync(w.keys, 0, (size_t)n_clusters * 8, s));
    dens_sizes_kernel<<<dim3(blocks256(a->n)), dim3(256), 0, s>>>(a->n, labels_dev, w.label, w.count, n_clusters, sizes_out_dev, w.keys);
    AVX_LAUNCH_CHECK();
    dens_exemplar_kernel<<<dim3((n_clusters + 255) / 256), dim3(256), 0, s>>>(n_clusters, w.keys, exemplar_out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
