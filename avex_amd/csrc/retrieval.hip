// Retrieval metrics on the device: the arithmetic behind avex/evaluation/retrieval.py (mean per-query ROC-AUC and precision@k over a
// cosine-similarity ranking), for embeddings that already live in HBM.
//
//   retr_normalize_kernel   rows / max(||row||_2, 1e-12) in fp32 (retrieval.py:242), written once with the width padded to the K tile
//   retr_pack_kernel        multi-hot label rows -> 64-bit words: relevance "shares an active class" (retrieval.py:152) is (a & b) != 0
//   retr_sim_kernel         S[b][n] = q^_b . d^_n on v_mfma_f32_32x32x2_f32: fp32 operands, one rounding per product (an f16-operand
//                           product moves the mean AUC by 1e-6 and flips precision@k hits).  The 128 x 128 x 32 LDS-DMA tile of f32_tile.h.
//   retr_rank_kernel        one workgroup per query row: relevance bits, top-k, and the Mann-Whitney count
//                               U2 = sum over (positive p, negative n) of 2 [s_p > s_n] + [s_p == s_n]          AUC = U2 / (2 P Q)
//                           as a 64-bit integer: exact for the similarities as computed, independent of any summation order.  The smaller
//                           of {positives, negatives} is sorted in LDS (bitonic, chunks of <= 16 Ki keys); every element of the other side
//                           does a lower- and an upper-bound search in it.
//   retr_finalize_kernel    validity rules of the reference + the fp64 means, in a fixed order (bit-reproducible).
// The top-k key is rank_key (f32_tile.h); reductions, sort and append are those of block_prims.h.
#include "block_prims.h"
#include "f32_tile.h"

namespace {

constexpr int RANK_THREADS = 256;
constexpr int RANK_MAX_K = 32;
constexpr int RANK_MAX_CAP = 16384;                // keys per sorted chunk (64 KiB of LDS)
constexpr int RETR_MAX_DB = 1 << 19;               // relevance bits of one row: 64 KiB of LDS

// ---------------------------------------------------------------------------------------------------------------------------------
// rows / max(||row||_2, 1e-12): f32_prepare_rows (f32_tile.h), which search.hip runs too
__global__ __launch_bounds__(256) void retr_normalize_kernel(const float* __restrict__ x, int64_t ldx, int n, int d, int dpad, float* __restrict__ out) {
    f32_prepare_rows(x, ldx, n, d, dpad, true, out);
}

__global__ __launch_bounds__(256) void retr_pack_kernel(const uint8_t* __restrict__ hot, int n, int c, int n_words, unsigned long long* __restrict__ words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * n_words) return;
    const int row = (int)(i / n_words), w = (int)(i - (int64_t)row * n_words);
    const uint8_t* r = hot + (int64_t)row * c;
    unsigned long long v = 0ull;
    const int hi = c - w * 64 < 64 ? c - w * 64 : 64;
    for (int b = 0; b < hi; ++b) v |= (unsigned long long)(r[w * 64 + b] != 0) << b;
    words[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// S[q][n] for q in [0, nq), n in [0, nd): Q and D are normalised rows of dpad floats (dpad % 32 == 0, zero beyond d).  The product is
// f32_tile_product with a store: f32_tile_store_product (f32_tile.h), which search.hip runs too.
__global__ __launch_bounds__(256) void retr_sim_kernel(const float* __restrict__ Q, int nq, const float* __restrict__ D, int nd, int dpad,
                                                        float* __restrict__ S, int64_t lds_) {
    f32_tile_store_product(Q, nq, D, nd, dpad, S, lds_);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct RankArgs {
    const float* S;
    int64_t lds_;
    int nd, self_base, n_words, k, cap;
    const int32_t* q_ids;
    const int32_t* d_ids;
    const unsigned long long* q_words;
    const unsigned long long* d_words;
    long long* u2;
    int32_t* stats;
    int32_t* topk;
};

// number of keys < x (LE = false) or <= x (LE = true) among the np2 ascending keys of a (np2 a power of two; the tail beyond the real
// keys is +inf).  Branch-free: the probe addresses of the first steps are the same in every lane (LDS broadcast).
template <bool LE> static __device__ __forceinline__ int count_below(const float* a, int np2, float x) {
    int lo = 0;
    for (int s = np2 >> 1; s >= 1; s >>= 1) {
        const float v = a[lo + s - 1];
        lo += (LE ? v <= x : v < x) ? s : 0;
    }
    const float v = a[lo];
    return lo + ((LE ? v <= x : v < x) ? 1 : 0);
}

__global__ __launch_bounds__(RANK_THREADS) void retr_rank_kernel(RankArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int WAVES = RANK_THREADS / 64;
    __shared__ unsigned long long red[5][WAVES];      // block_reduce has no trailing barrier: reductions back to back take a row each
    __shared__ int fill;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int b = blockIdx.x;
    const int nd = p.nd, k = p.k;
    const int self = p.self_base >= 0 ? p.self_base + b : -1;      // column of the query itself (self-set), never ranked
    const float* __restrict__ srow = p.S + (int64_t)b * p.lds_;
    const int nmw = (nd + 63) >> 6;
    unsigned long long* mask = (unsigned long long*)smem;                       // relevance bit of every column
    char* work = smem + (((size_t)nmw * 8 + 15) & ~(size_t)15);
    unsigned long long* list = (unsigned long long*)work;                       // [k][256] per-thread candidates, best first
    float* keys = (float*)work;                                                 // the sorted chunk (after the top-k is out)

    // ---- pass 1: relevance bits, positives, per-thread top-k candidates ---------------------------------------------------------
    for (int j = 0; j < k; ++j) list[j * RANK_THREADS + tid] = 0ull;
    unsigned long long thr = 0ull;
    int npos = 0, relself = 0;
    const int32_t qid = p.n_words == 0 ? p.q_ids[b] : 0;
    const unsigned long long* qw = p.q_words + (int64_t)b * p.n_words;
    for (int base = wid * 64; base < nd; base += RANK_THREADS) {      // wave-uniform trip count: the ballot sees all 64 lanes
        const int n = base + lane;
        const bool in = n < nd;
        bool rel = false;
        if (in) {
            if (p.n_words == 0) {
                rel = p.d_ids[n] == qid;
            } else {
                const unsigned long long* dw = p.d_words + (int64_t)n * p.n_words;
                unsigned long long any = 0ull;
                for (int w = 0; w < p.n_words; ++w) any |= dw[w] & qw[w];
                rel = any != 0ull;
            }
        }
        const unsigned long long bal = __ballot(rel);
        if (lane == 0) mask[base >> 6] = bal;
        if (in && n == self) relself = rel ? 1 : 0;
        if (in && n != self) {
            npos += rel ? 1 : 0;
            const unsigned long long key = rank_key(srow[n] + 0.0f, (unsigned)n);
            if (key > thr) {
                int j = k - 1;
                while (j > 0 && list[(j - 1) * RANK_THREADS + tid] < key) {
                    list[j * RANK_THREADS + tid] = list[(j - 1) * RANK_THREADS + tid];
                    --j;
                }
                list[j * RANK_THREADS + tid] = key;
                thr = list[(k - 1) * RANK_THREADS + tid];
            }
        }
    }
    const int P = (int)block_reduce<WAVES>((unsigned long long)npos, BlockSum(), red[0]);      // the barrier inside publishes mask[]
    const int rel_total = P + (int)block_reduce<WAVES>((unsigned long long)relself, BlockSum(), red[1]);
    const int n_eff = nd - ((self >= 0 && self < nd) ? 1 : 0);
    const int Q = n_eff - P;

    // ---- top-k: k rounds of "best head among the 256 sorted lists" --------------------------------------------------------------
    int head = 0, nhit = 0;
    for (int r = 0; r < RANK_MAX_K; ++r) {
        if (r >= k) {
            if (tid == 0) p.topk[(int64_t)b * RANK_MAX_K + r] = -1;
            continue;
        }
        const unsigned long long cur = head < k ? list[head * RANK_THREADS + tid] : 0ull;
        const unsigned long long best = block_reduce<WAVES>(cur, BlockMax(), red[2 + (r & 1)]);      // the rows alternate: the next round writes the other
        if (best != 0ull && cur == best) ++head;      // keys carry their column: unique
        if (tid == 0) {
            const int idx = best != 0ull ? (int)rank_key_index(best) : -1;
            p.topk[(int64_t)b * RANK_MAX_K + r] = idx;
            if (idx >= 0) nhit += (int)((mask[idx >> 6] >> (idx & 63)) & 1ull);
        }
    }
    if (tid == 0) {
        int32_t* st = p.stats + (int64_t)b * 4;
        st[0] = P;
        st[1] = Q;
        st[2] = rel_total;
        st[3] = nhit;
    }

    // ---- U2: sort the smaller side chunk by chunk, search with the larger -------------------------------------------------------
    unsigned long long u2 = 0ull;
    if (P > 0 && Q > 0) {
        const bool pos_small = P <= Q;
        const int m = pos_small ? P : Q;
        // a chunk is a column range that holds at most cap keys of the smaller side: every column when they all fit, cap columns otherwise
        const int cw = m <= p.cap ? ((nd + 63) & ~63) : p.cap;
        for (int c0 = 0; c0 < nd; c0 += cw) {
            __syncthreads();      // the previous chunk's searches (or the top-k lists) are done with `work`
            if (tid == 0) fill = 0;
            __syncthreads();
            const int c1 = c0 + cw < nd ? c0 + cw : nd;
            for (int base = c0 + wid * 64; base < c1; base += RANK_THREADS) {
                const int n = base + lane;
                const bool rel = (mask[base >> 6] >> lane) & 1ull;
                const bool sel = n < c1 && n != self && rel == pos_small;
                // the load is unconditional (a lane past the row reads its last column), so that it is in flight under the ballot and the
                // atomic; a chunk holds at most cap keys of the smaller side: the bound is a safety net that never rejects
                wave_append(sel, srow[n < nd ? n : nd - 1] + 0.0f, keys, &fill, p.cap);
            }
            __syncthreads();
            const int cnt = fill;
            if (cnt == 0) continue;      // block-uniform
            int np2 = 2;
            while (np2 < cnt) np2 <<= 1;
            for (int i = cnt + tid; i < np2; i += RANK_THREADS) keys[i] = __builtin_inff();
            __syncthreads();
            block_bitonic_sort<RANK_THREADS>(keys, np2, [](float a, float b) { return a < b; });      // ascending
            for (int base = wid * 64; base < nd; base += RANK_THREADS) {
                const int n = base + lane;
                const bool rel = (mask[base >> 6] >> lane) & 1ull;
                if (n < nd && n != self && rel != pos_small) {
                    const float x = srow[n] + 0.0f;
                    const int lb = count_below<false>(keys, np2, x);
                    int ub = lb;
                    if (lb < cnt && keys[lb] == x) ub = count_below<true>(keys, np2, x);      // ties are rare: one search for most elements
                    // sorted positives, x a negative: 2 (cnt - ub) wins + (ub - lb) ties; sorted negatives, x a positive: 2 lb + (ub - lb)
                    u2 += (unsigned long long)(pos_small ? 2 * cnt - ub - lb : lb + ub);
                }
            }
        }
    }
    const unsigned long long tot = block_reduce<WAVES>(u2, BlockSum(), red[4]);
    if (tid == 0) p.u2[b] = (long long)tot;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// out[0] = sum of per-query AUC over the valid queries, out[1] = their number, out[2] = sum of precision@k, out[3] = its number.
// Self-set (retrieval.py:262-284, 470-486): a query whose relevance vector, itself included, sums to <= 1 is skipped in both; so is, for
// the AUC, one with no negative left.  Cross-set (:386-399, 640-660): no positive = skipped in both; no negative = skipped in the AUC.
__global__ __launch_bounds__(256) void retr_finalize_kernel(const long long* __restrict__ u2, const int32_t* __restrict__ stats, int nq, int self_set,
                                                             int k, double* __restrict__ out) {
    typedef double f64x4 __attribute__((ext_vector_type(4)));      // the four sums as one value: one tree, each column in its own order
    __shared__ f64x4 red[256];
    const int tid = threadIdx.x;
    double a = 0.0, an = 0.0, pr = 0.0, pn = 0.0;
    for (int i = tid; i < nq; i += 256) {
        const int P = stats[4 * i], Q = stats[4 * i + 1], rt = stats[4 * i + 2], hit = stats[4 * i + 3];
        const bool vp = self_set ? rt > 1 : P > 0;
        const bool va = vp && P > 0 && Q > 0;
        if (va) {
            a += (double)u2[i] / (2.0 * (double)P * (double)Q);
            an += 1.0;
        }
        if (vp) {
            pr += (double)hit / (double)k;
            pn += 1.0;
        }
    }
    const f64x4 tot = block_tree_sum<256>((f64x4){a, an, pr, pn}, red);
    if (tid == 0)
        for (int c = 0; c < 4; ++c) out[c] = tot[c];
}

struct Workspace {
    float* dbn;
    float* qn;
    float* sim;
    size_t bytes;
};

static Workspace carve(void* ws, int64_t n_db, int d, int batch) {
    Workspace w;
    const size_t dp = (size_t)dpad_of(d);
    char* p = (char*)ws;
    w.dbn = take<float>(p, (size_t)n_db * dp);
    w.qn = take<float>(p, (size_t)batch * dp);
    w.sim = take<float>(p, (size_t)batch * (size_t)ldsim_of(n_db));
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

static size_t rank_lds_bytes(int nd, int k, int cap) {
    const size_t mask = ((size_t)((nd + 63) >> 6) * 8 + 15) & ~(size_t)15;
    const size_t lists = (size_t)k * RANK_THREADS * 8, keys = (size_t)cap * 4;
    return mask + (lists > keys ? lists : keys);
}

}  // namespace

extern "C" size_t avexhip_retrieval_workspace_bytes(int64_t n_db, int d, int batch, int n_words) {
    (void)n_words;      // packed labels are caller-owned buffers
    if (n_db <= 0 || d <= 0 || batch <= 0) return 0;
    return carve(nullptr, n_db, d, batch).bytes;
}

extern "C" int avexhip_retrieval_max_k(void) { return RANK_MAX_K; }

extern "C" int avexhip_retrieval_pack_labels(const uint8_t* multihot_dev, int n, int n_classes, uint64_t* words_dev, void* stream) {
    AVX_REQUIRE(multihot_dev && words_dev && n >= 0 && n_classes >= 1, "retrieval_pack_labels: bad arguments (n %d, classes %d)", n, n_classes);
    if (n == 0) return AVEXHIP_OK;
    const int nw = (n_classes + 63) / 64;
    const int64_t blocks = ((int64_t)n * nw + 255) / 256;
    AVX_REQUIRE(blocks <= 0x7fffffff, "retrieval_pack_labels: too many label words");
    retr_pack_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(multihot_dev, n, n_classes, nw, (unsigned long long*)words_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_retrieval_prepare(const float* db_dev, int64_t ld_db, int n_db, int d, int batch, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    AVX_REQUIRE(db_dev && workspace, "retrieval_prepare: null argument");
    AVX_REQUIRE(n_db >= 1 && n_db <= RETR_MAX_DB && d >= 1 && batch >= 1 && ld_db >= d, "retrieval_prepare: bad shape (n_db %d [1, %d], d %d, batch %d)",
                n_db, RETR_MAX_DB, d, batch);
    const Workspace w = carve(workspace, n_db, d, batch);
    if (workspace_bytes < w.bytes) {
        avexhip_set_error("retrieval_prepare: workspace %zu B < %zu B", workspace_bytes, w.bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    retr_normalize_kernel<<<dim3((n_db + 3) / 4), dim3(256), 0, (hipStream_t)stream>>>(db_dev, ld_db, n_db, d, (int)dpad_of(d), w.dbn);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_retrieval_batch(const avexhip_retrieval_args* a, void* stream) {
    AVX_REQUIRE(a && a->workspace && a->u2 && a->stats && a->topk, "retrieval_batch: null argument");
    AVX_REQUIRE(a->n_db >= 1 && a->n_db <= RETR_MAX_DB && a->d >= 1 && a->batch >= 1 && a->nb >= 1 && a->nb <= a->batch,
                "retrieval_batch: bad shape (n_db %d, d %d, batch %d, nb %d)", a->n_db, a->d, a->batch, a->nb);
    AVX_REQUIRE(a->k >= 1 && a->k <= RANK_MAX_K, "retrieval_batch: k %d outside [1, %d]", a->k, RANK_MAX_K);
    AVX_REQUIRE(a->n_words >= 0, "retrieval_batch: n_words %d", a->n_words);
    if (a->n_words == 0) AVX_REQUIRE(a->query_ids && a->db_ids, "retrieval_batch: class ids missing");
    else AVX_REQUIRE(a->query_words && a->db_words, "retrieval_batch: label words missing");
    if (a->self_set) AVX_REQUIRE(!a->query && a->q0 >= 0 && (int64_t)a->q0 + a->nb <= a->n_db, "retrieval_batch: self-set rows [%d, +%d) outside the database", a->q0, a->nb);
    else AVX_REQUIRE(a->query && a->ld_query >= a->d, "retrieval_batch: query rows missing");
    const Workspace w = carve(a->workspace, a->n_db, a->d, a->batch);
    if (a->workspace_bytes < w.bytes) {
        avexhip_set_error("retrieval_batch: workspace %zu B < %zu B", a->workspace_bytes, w.bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int dp = (int)dpad_of(a->d);
    const int64_t lds_ = ldsim_of(a->n_db);
    const int stages = a->stages == 0 ? 3 : a->stages;
    if (stages & 1) {
        const float* qn = w.dbn + (int64_t)a->q0 * dp;
        if (!a->self_set) {
            retr_normalize_kernel<<<dim3((a->nb + 3) / 4), dim3(256), 0, s>>>(a->query, a->ld_query, a->nb, a->d, dp, w.qn);
            AVX_LAUNCH_CHECK();
            qn = w.qn;
        }
        AVX_ENSURE_LDS(retr_sim_kernel, FT_LDS_BYTES);
        const dim3 grid((a->n_db + FT_BN - 1) / FT_BN, (a->nb + FT_BM - 1) / FT_BM);
        retr_sim_kernel<<<grid, dim3(256), FT_LDS_BYTES, s>>>(qn, a->nb, w.dbn, a->n_db, dp, w.sim, lds_);
        AVX_LAUNCH_CHECK();
        if (a->sim_out) {
            AVX_REQUIRE(a->ld_sim >= a->n_db, "retrieval_batch: ld_sim %lld < n_db", (long long)a->ld_sim);
            AVX_HIP_CHECK(hipMemcpy2DAsync(a->sim_out, (size_t)a->ld_sim * 4, w.sim, (size_t)lds_ * 4, (size_t)a->n_db * 4, (size_t)a->nb,
                                           hipMemcpyDeviceToDevice, s));
        }
    }
    if (stages & 2) {
        RankArgs r;
        r.S = w.sim;
        r.lds_ = lds_;
        r.nd = a->n_db;
        r.self_base = a->self_set ? a->q0 : -1;
        r.n_words = a->n_words;
        r.k = a->k;
        int cap = 64;      // the smaller side has at most n_db / 2 keys
        while (cap < (a->n_db + 1) / 2 && cap < RANK_MAX_CAP) cap <<= 1;
        r.cap = cap;
        r.q_ids = a->query_ids;
        r.d_ids = a->db_ids;
        r.q_words = (const unsigned long long*)a->query_words;
        r.d_words = (const unsigned long long*)a->db_words;
        r.u2 = (long long*)a->u2;
        r.stats = a->stats;
        r.topk = a->topk;
        const size_t lds = rank_lds_bytes(a->n_db, a->k, cap);
        AVX_ENSURE_LDS(retr_rank_kernel, rank_lds_bytes(RETR_MAX_DB, RANK_MAX_K, RANK_MAX_CAP));
        retr_rank_kernel<<<dim3(a->nb), dim3(RANK_THREADS), lds, s>>>(r);
        AVX_LAUNCH_CHECK();
    }
    return AVEXHIP_OK;
}

extern "C" int avexhip_retrieval_finalize(const int64_t* u2_dev, const int32_t* stats_dev, int n_query, int self_set, int k, double* out_dev,
                                          void* stream) {
    AVX_REQUIRE(u2_dev && stats_dev && out_dev && n_query >= 0 && k >= 1, "retrieval_finalize: bad arguments");
    retr_finalize_kernel<<<dim3(1), dim3(256), 0, (hipStream_t)stream>>>((const long long*)u2_dev, stats_dev, n_query, self_set, k, out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
