// Query-by-example search over embeddings that live in HBM: exact top-k of a query batch against a database held as a list of chunks.
//
//   srch_prepare_kernel   rows -> rows of dpad floats: divided by max(||row||_2, 1e-12) (cosine; the arithmetic of retr_normalize_kernel,
//                         retrieval.hip) or copied (dot).  Used once per database row when it is added, and per query batch.
//   srch_sim_kernel       S[b][n] = q_b . d_n for one query batch against one chunk: f32_tile_product (f32_tile.h) with a store, the shape
//                         of retr_sim_kernel.  The sum of a similarity runs over its two rows in an order the tile fixes: it does not depend
//                         on the chunk, the batch or the tile the pair falls in.
//   srch_select_kernel    one workgroup per query: the running list of the K' best keys merged with the chunk's similarities; a key is
//                         rank_key(similarity, global row) (f32_tile.h): higher similarity first, then lower row.  Keys are unique, so
//                         "the K' largest keys of everything seen so far" is one set, whatever the chunking, and the list is that set in
//                         descending order: the result does not depend on how the rows were split into chunks.
//                         Pass 0 forms the keys and drops columns (NaN, the query's own row, the exclusion rule, keys under the list's
//                         last entry when the list is full) by overwriting their similarity in the workspace with NaN.  A radix select on
//                         the key (8 bits per pass, most significant first, a histogram in LDS, stops as soon as a bucket is taken whole)
//                         finds the K'-th largest key of chunk + list; the keys at or above it are compacted into LDS and sorted (bitonic).
//                         Cost per chunk and query: O(columns) per radix pass, O(K' log^2 K') for the sort; nothing grows with k but the sort.
//                         LDS integer atomics only count (histogram bins, compaction slots); the sort of unique keys removes the slot order.
//   srch_finish_kernel    one workgroup per query: greedy temporal non-maximum suppression over the K' candidates (optional), then keys ->
//                         scores (the similarity's bits), rows, and the hits' recording / start / end.
#include "block_prims.h"
#include "f32_tile.h"

namespace {

constexpr int SRCH_THREADS = 256;
constexpr int SRCH_MAX_K = 1024;
constexpr int64_t SRCH_MAX_ROWS = 0x7fffffffll;      // global rows are the low 32 key bits, inverted

// ---------------------------------------------------------------------------------------------------------------------------------
// f32_prepare_rows and f32_tile_store_product (f32_tile.h) are the bodies of retr_normalize_kernel and retr_sim_kernel too
__global__ __launch_bounds__(256) void srch_prepare_kernel(const float* __restrict__ x, int64_t ldx, int n, int d, int dpad, int normalise,
                                                           float* __restrict__ out) {
    f32_prepare_rows(x, ldx, n, d, dpad, normalise != 0, out);
}

// S[q][n] for q in [0, nq), n in [0, nd): Q and D are prepared rows of dpad floats (dpad % 32 == 0, zero beyond d)
__global__ __launch_bounds__(256) void srch_sim_kernel(const float* __restrict__ Q, int nq, const float* __restrict__ D, int nd, int dpad,
                                                       float* __restrict__ S, int64_t lds_) {
    f32_tile_store_product(Q, nq, D, nd, dpad, S, lds_);
}

__global__ __launch_bounds__(256) void srch_reset_kernel(unsigned long long* __restrict__ lists, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) lists[i] = 0ull;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct SelectArgs {
    float* S;                       // [nb][lds_]: this chunk's similarities; dropped columns are overwritten with NaN
    int64_t lds_;
    int nd, kp, exclude;
    unsigned row0;                  // global row of column 0
    unsigned long long* lists;      // [nb][kp] keys, descending, 0 = empty
    const int64_t* skip_row;        // [nb] or NULL
    const int32_t* q_rec;           // [nb]           (exclude != 0)
    const double* q_start;          // [nb]           (exclude == 2)
    const double* q_end;
    const int32_t* d_rec;           // [nd] of this chunk
    const double* d_start;
    const double* d_end;
};

// min / max of two spans' ends as np.minimum / np.maximum give them: a NaN on either side is the result, so every compare that follows is
// false and a row without a span (NaN) neither excludes, nor is excluded, nor suppresses, nor is suppressed
static __device__ __forceinline__ double srch_min(double a, double b) { return (a < b || a != a) ? a : b; }
static __device__ __forceinline__ double srch_max(double a, double b) { return (a > b || a != a) ? a : b; }

// The entries of a descending key list are a prefix: the first index in [0, n) that holds 0 (n when none does), by a search every thread
// makes for itself (the same addresses in every lane)
static __device__ __forceinline__ int srch_entries(const unsigned long long* list, int n) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] != 0ull) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SRCH_THREADS) void srch_select_kernel(SelectArgs p) {
    __shared__ unsigned long long old_[SRCH_MAX_K];
    __shared__ unsigned long long surv[SRCH_MAX_K];
    __shared__ int hist[256];
    __shared__ int wsum[SRCH_THREADS / 64];
    __shared__ int fill;
    __shared__ int sel_digit, sel_above;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int b = blockIdx.x;
    const int nd = p.nd, kp = p.kp;
    float* __restrict__ srow = p.S + (int64_t)b * p.lds_;
    unsigned long long* __restrict__ list = p.lists + (int64_t)b * kp;

    for (int i = tid; i < kp; i += SRCH_THREADS) old_[i] = list[i];
    if (tid == 0) fill = 0;      // the compaction's counter, published by this barrier
    __syncthreads();
    const int n_old = srch_entries(old_, kp);
    const unsigned long long floor_key = n_old == kp ? old_[kp - 1] : 0ull;      // a full list: nothing under its last entry can enter

    // ---- pass 0: drop columns, count the rest -------------------------------------------------------------------------------------
    const long long skip = p.skip_row ? p.skip_row[b] : -1ll;
    const int qrec = p.exclude ? p.q_rec[b] : -1;
    const double qs = p.exclude == 2 ? p.q_start[b] : 0.0, qe = p.exclude == 2 ? p.q_end[b] : 0.0;
    int mine = 0;
    for (int n = tid; n < nd; n += SRCH_THREADS) {
        const float s = srow[n];
        if (s != s) continue;
        const unsigned grow = p.row0 + (unsigned)n;
        bool drop = (long long)grow == skip;
        if (!drop && qrec >= 0 && p.d_rec[n] == qrec) {
            if (p.exclude == 1) {
                drop = true;
            } else {
                const double ds = p.d_start[n], de = p.d_end[n];
                drop = srch_min(qe, de) > srch_max(qs, ds);      // a positive overlap: min(end) > max(start), no arithmetic
            }
        }
        if (!drop) drop = rank_key(s + 0.0f, grow) < floor_key;
        if (drop) srow[n] = __builtin_nanf("");
        else ++mine;
    }
    const int n_new = block_reduce<SRCH_THREADS / 64>(mine, BlockSum(), wsum);
    if (n_new == 0) return;      // block-uniform: the list stands
    const int total = n_new + n_old;

    // ---- the kp-th largest key of chunk + list (every key when there are no more than kp) -----------------------------------------
    unsigned long long thr = 0ull;      // keys >= thr survive; every real key is > 0
    if (total > kp) {
        unsigned long long prefix = 0ull;
        int need = kp;
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            hist[tid] = 0;
            __syncthreads();
            for (int n = tid; n < nd; n += SRCH_THREADS) {
                const float s = srow[n];
                if (s != s) continue;
                const unsigned long long key = rank_key(s + 0.0f, p.row0 + (unsigned)n);
                if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
            }
            for (int i = tid; i < n_old; i += SRCH_THREADS) {
                const unsigned long long key = old_[i];
                if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
            }
            __syncthreads();
            // digit tid is the one when the bins above it hold < need keys and the bins from it on hold >= need
            int above = 0;
            for (int d = 255; d > tid; --d) above += hist[d];
            if (above < need && above + hist[tid] >= need) {
                sel_digit = tid;
                sel_above = above;
            }
            __syncthreads();
            const int dg = sel_digit;
            need -= sel_above;
            prefix = (prefix << 8) | (unsigned long long)dg;
            const bool whole = hist[dg] == need;      // the bucket is taken whole: its smallest possible key is the threshold
            __syncthreads();                           // hist and sel_* are read; the next pass may reset them
            if (whole || pass == 7) {
                thr = prefix << shift;
                break;
            }
        }
    }

    // ---- compaction of the survivors, then a descending bitonic sort ---------------------------------------------------------------
    const int n_keep = total > kp ? kp : total;
    for (int base = wid * 64; base < nd; base += SRCH_THREADS) {      // wave-uniform trip count: the ballot sees all 64 lanes
        const int n = base + lane;
        unsigned long long key = 0ull;
        if (n < nd) {
            const float s = srow[n];
            if (s == s) key = rank_key(s + 0.0f, p.row0 + (unsigned)n);
        }
        wave_append(key != 0ull && key >= thr, key, surv, &fill, SRCH_MAX_K);
    }
    for (int base = wid * 64; base < n_old; base += SRCH_THREADS) {
        const int i = base + lane;
        const unsigned long long key = i < n_old ? old_[i] : 0ull;
        wave_append(key != 0ull && key >= thr, key, surv, &fill, SRCH_MAX_K);
    }
    __syncthreads();
    int np2 = 2;
    while (np2 < n_keep) np2 <<= 1;
    for (int i = n_keep + tid; i < np2; i += SRCH_THREADS) surv[i] = 0ull;
    __syncthreads();
    block_bitonic_sort<SRCH_THREADS>(surv, np2, [](unsigned long long a, unsigned long long b) { return a > b; });      // descending
    for (int i = tid; i < kp; i += SRCH_THREADS) list[i] = i < n_keep ? surv[i] : 0ull;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct FinishArgs {
    const unsigned long long* lists;      // [nb][kp]
    int kp, k, nms;
    double max_overlap;
    long long n_rows;                     // rows of the index: metadata is read for rows below it only
    const int32_t* d_rec;                 // [n_rows] or NULL
    const double* d_start;
    const double* d_end;
    float* scores;                        // [nb][k]
    int64_t* rows;
    int32_t* count;                       // [nb]
    int32_t* rec;                         // [nb][k]
    double* start;
    double* end;
};

__global__ __launch_bounds__(SRCH_THREADS) void srch_finish_kernel(FinishArgs p) {
    __shared__ int32_t c_rec[SRCH_MAX_K];
    __shared__ double c_start[SRCH_MAX_K];
    __shared__ double c_end[SRCH_MAX_K];
    __shared__ short kept[SRCH_MAX_K];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int kp = p.kp, k = p.k;
    const unsigned long long* __restrict__ list = p.lists + (int64_t)b * kp;
    const double nan = __builtin_nan("");

    for (int i = tid; i < kp; i += SRCH_THREADS) {
        const unsigned long long key = list[i];
        const long long row = (long long)rank_key_index(key);
        const bool meta = key != 0ull && row < p.n_rows && p.d_rec != nullptr;
        c_rec[i] = meta ? p.d_rec[row] : -1;
        c_start[i] = meta ? p.d_start[row] : nan;
        c_end[i] = meta ? p.d_end[row] : nan;
    }
    __syncthreads();

    int n_kept = 0;
    if (!p.nms) {
        n_kept = srch_entries(list, kp < k ? kp : k);
        for (int i = tid; i < n_kept; i += SRCH_THREADS) kept[i] = (short)i;
    } else {
        // best first: a candidate falls when a hit already kept is of its recording and overlaps it by more than max_overlap x the shorter
        // of the two.  Both sides of the compare are rounded on their own (no fused multiply-add can form across a compare).
        for (int c = 0; c < kp && n_kept < k; ++c) {
            if (list[c] == 0ull) break;              // block-uniform
            const int rc = c_rec[c];
            int hit = 0;
            if (rc >= 0) {
                const double sc = c_start[c], ec = c_end[c], lc = ec - sc;
                for (int j = tid; j < n_kept; j += SRCH_THREADS) {
                    const int o = kept[j];
                    if (c_rec[o] != rc) continue;
                    const double so = c_start[o], eo = c_end[o], lo_ = eo - so;
                    const double inter = srch_min(ec, eo) - srch_max(sc, so);
                    const double bound = p.max_overlap * srch_min(lc, lo_);
                    if (inter > bound) hit = 1;
                }
            }
            hit = __syncthreads_or(hit);
            if (!hit) {
                if (tid == 0) kept[n_kept] = (short)c;
                ++n_kept;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0) p.count[b] = n_kept;
    for (int j = tid; j < k; j += SRCH_THREADS) {
        const int64_t o = (int64_t)b * k + j;
        if (j < n_kept) {
            const int c = kept[j];
            const unsigned long long key = list[c];
            p.scores[o] = rank_key_value(key);
            p.rows[o] = (int64_t)rank_key_index(key);
            p.rec[o] = c_rec[c];
            p.start[o] = c_start[c];
            p.end[o] = c_end[c];
        } else {
            p.scores[o] = -__builtin_inff();
            p.rows[o] = -1;
            p.rec[o] = -1;
            p.start[o] = nan;
            p.end[o] = nan;
        }
    }
}

struct Workspace {
    float* qn;
    float* sim;
    unsigned long long* lists;
    size_t bytes;
};

static Workspace carve(void* ws, int64_t chunk_rows, int d, int batch, int k) {
    Workspace w;
    char* p = (char*)ws;
    w.qn = take<float>(p, (size_t)batch * (size_t)dpad_of(d));
    w.sim = take<float>(p, (size_t)batch * (size_t)ldsim_of(chunk_rows));
    w.lists = take<unsigned long long>(p, (size_t)batch * (size_t)k);
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

static bool shape_ok(const avexhip_search_args* a) {
    return a->chunk_rows >= 1 && a->d >= 1 && a->batch >= 1 && a->nb >= 1 && a->nb <= a->batch && a->k >= 1 && a->k <= SRCH_MAX_K;
}

}  // namespace

extern "C" int avexhip_search_max_k(void) { return SRCH_MAX_K; }

extern "C" size_t avexhip_search_workspace_bytes(int64_t chunk_rows, int d, int batch, int k) {
    if (chunk_rows <= 0 || chunk_rows > SRCH_MAX_ROWS || d <= 0 || batch <= 0 || k <= 0 || k > SRCH_MAX_K) return 0;
    return carve(nullptr, chunk_rows, d, batch, k).bytes;
}

extern "C" int avexhip_search_prepare_rows(const float* rows_dev, int64_t ld_rows, int n, int d, int normalise, float* out_dev, void* stream) {
    AVX_REQUIRE(rows_dev && out_dev, "search_prepare_rows: null argument");
    AVX_REQUIRE(n >= 0 && d >= 1 && ld_rows >= d, "search_prepare_rows: bad shape (n %d, d %d, ld_rows %lld)", n, d, (long long)ld_rows);
    AVX_REQUIRE(normalise == 0 || normalise == 1, "search_prepare_rows: normalise %d is neither 0 nor 1", normalise);
    if (n == 0) return AVEXHIP_OK;
    srch_prepare_kernel<<<dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream>>>(rows_dev, ld_rows, n, d, (int)dpad_of(d), normalise, out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_search_begin(const avexhip_search_args* a, void* stream) {
    AVX_REQUIRE(a && a->workspace && a->query, "search_begin: null argument");
    AVX_REQUIRE(shape_ok(a), "search_begin: bad shape (chunk_rows %lld, d %d, batch %d, nb %d, k %d [1, %d])", (long long)a->chunk_rows, a->d, a->batch,
                a->nb, a->k, SRCH_MAX_K);
    AVX_REQUIRE(a->ld_query >= a->d, "search_begin: ld_query %lld < d %d", (long long)a->ld_query, a->d);
    AVX_REQUIRE(a->normalise == 0 || a->normalise == 1, "search_begin: normalise %d is neither 0 nor 1", a->normalise);
    const Workspace w = carve(a->workspace, a->chunk_rows, a->d, a->batch, a->k);
    if (a->workspace_bytes < w.bytes) {
        avexhip_set_error("search_begin: workspace %zu B < %zu B", a->workspace_bytes, w.bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    srch_prepare_kernel<<<dim3((a->nb + 3) / 4), dim3(256), 0, s>>>(a->query, a->ld_query, a->nb, a->d, (int)dpad_of(a->d), a->normalise, w.qn);
    AVX_LAUNCH_CHECK();
    const int64_t n = (int64_t)a->nb * a->k;
    srch_reset_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(w.lists, n);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_search_chunk(const avexhip_search_args* a, void* stream) {
    AVX_REQUIRE(a && a->workspace && a->chunk, "search_chunk: null argument");
    AVX_REQUIRE(shape_ok(a), "search_chunk: bad shape (chunk_rows %lld, d %d, batch %d, nb %d, k %d [1, %d])", (long long)a->chunk_rows, a->d, a->batch,
                a->nb, a->k, SRCH_MAX_K);
    AVX_REQUIRE(a->n_rows >= 1 && a->n_rows <= a->chunk_rows, "search_chunk: %d rows in a chunk of %lld", a->n_rows, (long long)a->chunk_rows);
    AVX_REQUIRE(a->row0 >= 0 && a->row0 + a->n_rows <= SRCH_MAX_ROWS, "search_chunk: rows [%lld, +%d) leave 0 .. 2^31 - 2", (long long)a->row0, a->n_rows);
    AVX_REQUIRE(a->exclude >= 0 && a->exclude <= 2, "search_chunk: exclude %d outside 0 .. 2", a->exclude);
    if (a->exclude >= 1) AVX_REQUIRE(a->query_recording && a->db_recording, "search_chunk: exclude %d without the recordings", a->exclude);
    if (a->exclude == 2) AVX_REQUIRE(a->query_start && a->query_end && a->db_start && a->db_end, "search_chunk: exclude 2 without the spans");
    if (a->sim_out) AVX_REQUIRE(a->ld_sim >= a->n_rows, "search_chunk: ld_sim %lld < %d rows", (long long)a->ld_sim, a->n_rows);
    const Workspace w = carve(a->workspace, a->chunk_rows, a->d, a->batch, a->k);
    if (a->workspace_bytes < w.bytes) {
        avexhip_set_error("search_chunk: workspace %zu B < %zu B", a->workspace_bytes, w.bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int dp = (int)dpad_of(a->d);
    const int64_t lds_ = ldsim_of(a->chunk_rows);
    const int stages = a->stages == 0 ? 3 : a->stages;
    AVX_REQUIRE(stages >= 1 && stages <= 3, "search_chunk: stages %d outside 0 .. 3", a->stages);
    if (stages & 1) {
        AVX_ENSURE_LDS(srch_sim_kernel, FT_LDS_BYTES);
        const dim3 grid((a->n_rows + FT_BN - 1) / FT_BN, (a->nb + FT_BM - 1) / FT_BM);
        srch_sim_kernel<<<grid, dim3(256), FT_LDS_BYTES, s>>>(w.qn, a->nb, a->chunk, a->n_rows, dp, w.sim, lds_);
        AVX_LAUNCH_CHECK();
        if (a->sim_out)
            AVX_HIP_CHECK(hipMemcpy2DAsync(a->sim_out, (size_t)a->ld_sim * 4, w.sim, (size_t)lds_ * 4, (size_t)a->n_rows * 4, (size_t)a->nb,
                                           hipMemcpyDeviceToDevice, s));
    }
    if (stages & 2) {
        SelectArgs r;
        r.S = w.sim;
        r.lds_ = lds_;
        r.nd = a->n_rows;
        r.kp = a->k;
        r.exclude = a->exclude;
        r.row0 = (unsigned)a->row0;
        r.lists = w.lists;
        r.skip_row = a->skip_row;
        r.q_rec = a->query_recording;
        r.q_start = a->query_start;
        r.q_end = a->query_end;
        r.d_rec = a->db_recording;
        r.d_start = a->db_start;
        r.d_end = a->db_end;
        srch_select_kernel<<<dim3(a->nb), dim3(SRCH_THREADS), 0, s>>>(r);
        AVX_LAUNCH_CHECK();
    }
    return AVEXHIP_OK;
}

extern "C" int avexhip_search_finish(const avexhip_search_args* a, const avexhip_search_result* r, void* stream) {
    AVX_REQUIRE(a && r && a->workspace, "search_finish: null argument");
    AVX_REQUIRE(shape_ok(a), "search_finish: bad shape (chunk_rows %lld, d %d, batch %d, nb %d, k %d [1, %d])", (long long)a->chunk_rows, a->d, a->batch,
                a->nb, a->k, SRCH_MAX_K);
    AVX_REQUIRE(r->scores && r->rows && r->count && r->recording && r->start_s && r->end_s, "search_finish: null output");
    AVX_REQUIRE(r->k >= 1 && r->k <= a->k, "search_finish: k %d outside [1, %d], the depth of the lists", r->k, a->k);
    AVX_REQUIRE(r->nms == 0 || r->nms == 1, "search_finish: nms %d is neither 0 nor 1", r->nms);
    if (r->nms) AVX_REQUIRE(r->max_overlap >= 0.0 && r->max_overlap < 1.0, "search_finish: max_overlap %g outside [0, 1)", r->max_overlap);
    else AVX_REQUIRE(r->k == a->k, "search_finish: k %d != the depth of the lists %d without suppression", r->k, a->k);
    AVX_REQUIRE(r->n_rows >= 0 && r->n_rows <= SRCH_MAX_ROWS, "search_finish: %lld rows outside 0 .. 2^31 - 1", (long long)r->n_rows);
    if (r->db_recording) AVX_REQUIRE(r->db_start && r->db_end, "search_finish: recordings without the spans");
    const Workspace w = carve(a->workspace, a->chunk_rows, a->d, a->batch, a->k);
    if (a->workspace_bytes < w.bytes) {
        avexhip_set_error("search_finish: workspace %zu B < %zu B", a->workspace_bytes, w.bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    FinishArgs f;
    f.lists = w.lists;
    f.kp = a->k;
    f.k = r->k;
    f.nms = r->nms;
    f.max_overlap = r->max_overlap;
    f.n_rows = r->n_rows;
    f.d_rec = r->db_recording;
    f.d_start = r->db_start;
    f.d_end = r->db_end;
    f.scores = r->scores;
    f.rows = r->rows;
    f.count = r->count;
    f.rec = r->recording;
    f.start = r->start_s;
    f.end = r->end_s;
    srch_finish_kernel<<<dim3(a->nb), dim3(SRCH_THREADS), 0, (hipStream_t)stream>>>(f);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
