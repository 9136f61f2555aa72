// Clustering metrics on the device: the arithmetic behind avex/evaluation/clustering.py -- scikit-learn's seeded KMeans (greedy k-means++,
// n_init restarts of Lloyd's algorithm) and the three scores ARI / NMI / V-measure -- for embeddings that already live in HBM.
//
// All R = n_init restarts advance in lock-step: every stage is one launch over all of them, X is streamed once per stage, and the
// assign product sees R * kpad centre columns (kpad = k rounded up to 32: a 32-lane column group of the MFMA result then belongs to one
// restart).  The random numbers (a few hundred doubles) come from the host's numpy RandomState; everything that touches the data is here.
//
//   clus_colsum / mean / centre / tol / rownorm   column means (fp64 partial sums in a fixed order), X - mean written once with the width padded
//                           to the K tile, tol_abs = mean(var(X, axis 0)) * tol, row norms, the finite flag
//   clus_seed_dist_kernel   k-means++ step: squared distances from the R * (2 + int(ln k)) candidate rows to every point, direct differences
//                           summed over the columns in ascending order (fp32, no FMA contraction: reproducible in NumPy bit for bit), min with
//                           the running closest distance
//   clus_seed_pick_kernel   one workgroup per restart: candidate potentials (fp64), arg-min (first on ties), the new centre; then the fp64 prefix
//                           sum of the closest distances and a left binary search per draw = the next step's candidate rows
//   clus_assign_kernel      argmin_j (||c_j||^2 - 2 x.c_j) on v_mfma_f32_32x32x2_f32 (exact fp32 operands): the 128 x 128 x 32 LDS-DMA tile of
//                           f32_tile.h, which retr_sim_kernel (retrieval.hip) uses too, with a reducing epilogue: a 5-step butterfly over the
//                           32 lanes that hold one row's columns, then a 64-bit atomicMin of (monotone(dist) << 32 | j) -- order-free, first
//                           minimum on ties.  The N x R k distance matrix is never written.
//   clus_post_kernel        labels out of the packed minima, number of changed labels (integer atomics)
//   clus_update_kernel      per (restart, cluster): the sum of its rows IN ASCENDING ROW ORDER (labels compacted tile by tile, then a sequential
//                           fp32 sum: bit-reproducible, no float atomics) and the count
//   clus_relocate_kernel    scikit-learn's empty-cluster rule: the e points farthest from their assigned centre, largest first, become the e
//                           empty clusters (ascending id); labels are not changed in that iteration
//   clus_decide_kernel      centre = sum * (1 / count), shift = sum (new - old)^2, and the stopping rules per restart: labels unchanged (strict,
//                           new centres kept) or shift <= tol_abs / max_iter reached (one more assign); a finished restart is frozen
//   clus_inertia / select / export   sum ||x - c_label||^2 (fp32 terms, fp64 sums in a fixed order), the first strictly smallest, its labels and
//                           centres (mean added back)
//   clus_contingency / scores   integer contingency table, then ARI / NMI / V-measure in fp64 by scikit-learn's formulas
//
// Limits: k <= 4096, n_init <= 64, n <= 2^24.
#include "block_prims.h"
#include "f32_tile.h"

namespace {

constexpr int CLUS_MAX_K = 4096, CLUS_MAX_INIT = 64, CLUS_MAX_N = 1 << 24;
constexpr int CLUS_MAX_TRIALS = 12;                // 2 + int(ln 4096) = 10
constexpr int NCHUNK = 128;                        // row chunks of the column reductions
constexpr int SG = 16;                             // candidates per seed_dist workgroup
constexpr unsigned long long KEY_NONE = ~0ull;

static inline int kpad_of(int k) { return (k + 31) / 32 * 32; }
static inline int trials_of(int k) {
    int t = 2;      // 2 + int(ln k) without floating point on the boundary: ln k >= m  <=>  k >= ceil(e^m)
    static const int ceil_exp[] = {3, 8, 21, 55, 149, 404, 1097, 2981, 8104};
    for (int m = 0; m < 9 && k >= ceil_exp[m]; ++m) ++t;
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------------------
//  Stage 1: centre, norms, tolerance, finite flag
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clus_colsum_kernel(const float* __restrict__ x, int64_t ldx, int n, int d, int dpad, int rows_per,
                                                           double* __restrict__ part, int32_t* __restrict__ nonfinite) {
    const int col = blockIdx.y * 256 + threadIdx.x;
    if (col >= dpad) return;
    const int r0 = blockIdx.x * rows_per;
    const int r1 = r0 + rows_per < n ? r0 + rows_per : n;
    double s = 0.0;
    bool bad = false;
    if (col < d)
        for (int r = r0; r < r1; ++r) {
            const float v = x[(int64_t)r * ldx + col];
            bad |= !(__builtin_fabsf(v) <= 3.4028234663852886e38f);
            s += (double)v;
        }
    part[(int64_t)blockIdx.x * dpad + col] = s;
    if (bad) atomicOr(nonfinite, 1);
}

__global__ __launch_bounds__(256) void clus_mean_kernel(const double* __restrict__ part, int n, int d, int dpad, float* __restrict__ mean) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= dpad) return;
    double s = 0.0;
    for (int c = 0; c < NCHUNK; ++c) s += part[(int64_t)c * dpad + col];
    mean[col] = col < d ? (float)(s / (double)n) : 0.f;
}

__global__ __launch_bounds__(256) void clus_centre_kernel(const float* __restrict__ x, int64_t ldx, int n, int d, int dpad, int rows_per,
                                                           const float* __restrict__ mean, float* __restrict__ xc, double* __restrict__ part) {
    const int col = blockIdx.y * 256 + threadIdx.x;
    if (col >= dpad) return;
    const int r0 = blockIdx.x * rows_per;
    const int r1 = r0 + rows_per < n ? r0 + rows_per : n;
    const float m = mean[col];
    double s = 0.0;
    for (int r = r0; r < r1; ++r) {
        const float v = col < d ? x[(int64_t)r * ldx + col] - m : 0.f;
        xc[(int64_t)r * dpad + col] = v;
        s += (double)v * (double)v;
    }
    part[(int64_t)blockIdx.x * dpad + col] = s;
}

__global__ __launch_bounds__(256) void clus_tol_kernel(const double* __restrict__ part, int n, int d, int dpad, double tol, double* __restrict__ tol_abs) {
    __shared__ double red[256];
    double s = 0.0;
    for (int col = threadIdx.x; col < d; col += 256) {
        double c = 0.0;
        for (int ch = 0; ch < NCHUNK; ++ch) c += part[(int64_t)ch * dpad + col];
        s += c / (double)n;
    }
    const double tot = block_tree_sum<256>(s, red);
    if (threadIdx.x == 0) tol_abs[0] = tot / (double)d * tol;
}

__global__ __launch_bounds__(256) void clus_rownorm_kernel(const float* __restrict__ xc, int n, int dpad, float* __restrict__ xnorm) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const f32x4* r = (const f32x4*)(xc + (int64_t)row * dpad);
    float s = 0.f;
    for (int c = 0; c < dpad / 4; ++c) {
        const f32x4 v = r[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) s = s + v[e] * v[e];
    }
    xnorm[row] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
//  Stage 2: k-means++ seeding
// ---------------------------------------------------------------------------------------------------------------------------------
// mind[ci][row] = min(closest[ci / T][row], ||x_row - x_cand[ci]||^2) for the SG candidates of this workgroup (first: no min, T = 1).
// One thread per point; the candidates' K tile sits in LDS (every lane reads the same address: broadcast).
__global__ __launch_bounds__(256) void clus_seed_dist_kernel(const float* __restrict__ xc, int n, int dpad, const int32_t* __restrict__ cand, int n_cand,
                                                              int T, int first, const float* __restrict__ closest, float* __restrict__ mind) {
    __shared__ __attribute__((aligned(16))) float tile[SG][FT_BK];
    const int tid = threadIdx.x;
    const int row = blockIdx.x * 256 + tid;
    const int g0 = blockIdx.y * SG;
    const int rr = row < n ? row : n - 1;
    const float* __restrict__ xr = xc + (int64_t)rr * dpad;
    float acc[SG];
#pragma unroll
    for (int g = 0; g < SG; ++g) acc[g] = 0.f;
    for (int k0 = 0; k0 < dpad; k0 += FT_BK) {
        __syncthreads();
        for (int e = tid; e < SG * FT_BK; e += 256) {
            const int g = e >> 5, c = e & 31;
            int id = g0 + g < n_cand ? cand[g0 + g] : 0;
            id = id < 0 ? 0 : (id >= n ? n - 1 : id);
            tile[g][c] = xc[(int64_t)id * dpad + k0 + c];
        }
        __syncthreads();
        f32x4 xv[FT_BK / 4];
#pragma unroll
        for (int c4 = 0; c4 < FT_BK / 4; ++c4) xv[c4] = *(const f32x4*)(xr + k0 + c4 * 4);
#pragma unroll
        for (int c4 = 0; c4 < FT_BK / 4; ++c4)
#pragma unroll
            for (int g = 0; g < SG; ++g) {
                const f32x4 t = *(const f32x4*)&tile[g][c4 * 4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float df = xv[c4][e] - t[e];
                    acc[g] = acc[g] + df * df;
                }
            }
    }
    if (row >= n) return;
#pragma unroll
    for (int g = 0; g < SG; ++g) {
        const int ci = g0 + g;
        if (ci < n_cand) {
            float v = acc[g];
            if (!first) {
                const float cl = closest[(int64_t)(ci / T) * n + row];
                v = cl < v ? cl : v;
            }
            mind[(int64_t)ci * n + row] = v;
        }
    }
}

// One workgroup per restart r, step c (the centre being chosen): potentials of the T_in candidates, the winner, its row as centre c; then the
// draws of step c + 1: cum = fp64 prefix sum of the winner's min-distances (which become `closest`), candidate = first index with
// cum >= u * potential, clipped to n - 1.
__global__ __launch_bounds__(1024) void clus_seed_pick_kernel(const float* __restrict__ xc, int n, int dpad, int k, int kpad, int c, int T_in, int T,
                                                               const double* __restrict__ u, float* __restrict__ mind, float* __restrict__ closest,
                                                               double* __restrict__ cum, int32_t* __restrict__ cand, int32_t* __restrict__ cand_next,
                                                               int32_t* __restrict__ seeds, float* __restrict__ centres) {
    __shared__ double red[1024];
    __shared__ double pots[CLUS_MAX_TRIALS];
    __shared__ int best_s;
    const int tid = threadIdx.x, r = blockIdx.x;
    for (int t = 0; t < T_in; ++t) {
        const float* __restrict__ m = mind + (int64_t)(r * T_in + t) * n;
        double s = 0.0;
        for (int i = tid; i < n; i += 1024) s += (double)m[i];
        const double tot = block_tree_sum<1024>(s, red);
        if (tid == 0) pots[t] = tot;
    }
    if (tid == 0) {
        int b = 0;
        for (int t = 1; t < T_in; ++t)
            if (pots[t] < pots[b]) b = t;
        best_s = b;
    }
    __syncthreads();
    const int best = best_s;
    const double pot = pots[best];
    int id = cand[r * T_in + best];
    id = id < 0 ? 0 : (id >= n ? n - 1 : id);
    if (tid == 0) seeds[r * k + c] = id;
    float* __restrict__ crow = centres + ((int64_t)r * kpad + c) * dpad;
    for (int col = tid; col < dpad; col += 1024) crow[col] = xc[(int64_t)id * dpad + col];
    if (c == k - 1) return;
    const float* __restrict__ m = mind + (int64_t)(r * T_in + best) * n;
    float* __restrict__ cl = closest + (int64_t)r * n;
    double* __restrict__ cm = cum + (int64_t)r * n;
    const int seg = (n + 1023) / 1024;
    const int i0 = tid * seg < n ? tid * seg : n;
    const int i1 = i0 + seg < n ? i0 + seg : n;
    double s = 0.0;
    for (int i = i0; i < i1; ++i) s += (double)m[i];
    red[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int t = 0; t < 1024; ++t) {
            const double v = red[t];
            red[t] = run;
            run += v;
        }
    }
    __syncthreads();
    double run = red[tid];
    for (int i = i0; i < i1; ++i) {
        const float v = m[i];
        run += (double)v;
        cm[i] = run;
        cl[i] = v;
    }
    __threadfence_block();
    __syncthreads();
    if (tid < T) {
        const double v = u[((int64_t)r * (k - 1) + c) * T + tid] * pot;
        int lo = 0, hi = n;      // first index with cm[index] >= v
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cm[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        cand_next[r * T + tid] = lo < n - 1 ? lo : n - 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
//  Stage 3: assign
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clus_cnorm_kernel(const float* __restrict__ centres, int rows, int dpad, float* __restrict__ cnorm) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const f32x4* r = (const f32x4*)(centres + (int64_t)row * dpad);
    float s = 0.f;
    for (int c = 0; c < dpad / 4; ++c) {
        const f32x4 v = r[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) s = s + v[e] * v[e];
    }
    cnorm[row] = s;
}

// best[rst][q] = min over the centres j of restart rst of (mono(||c_j||^2 - 2 x_q . c_j) << 32 | j).  X = points (rows of the MFMA result),
// C = the R * kpad centre rows (its columns).  The product is f32_tile_product (f32_tile.h).
__global__ __launch_bounds__(256) void clus_assign_kernel(const float* __restrict__ X, int nq, const float* __restrict__ Cn, int nd, int dpad, int k, int kpad,
                                                           const float* __restrict__ cnorm, const int32_t* __restrict__ status,
                                                           unsigned long long* __restrict__ best) {
    const int lane = threadIdx.x & 63;
    const int n0 = blockIdx.x * FT_BN, q0 = blockIdx.y * FT_BM;
    {      // a tile whose restarts are all finished has nothing to do (block-uniform, before any barrier)
        const int last = n0 + FT_BN - 1 < nd - 1 ? n0 + FT_BN - 1 : nd - 1;
        bool live = false;
        for (int rst = n0 / kpad; rst <= last / kpad; ++rst) live |= status[rst] != 2;
        if (!live) return;
    }
    f32x16 acc[2][2];
    f32_tile_product(X, nq, q0, Cn, nd, n0, dpad, acc);
    // The 32 lanes of a half wave hold the 32 columns of one row (f32_tile_row / f32_tile_col): a butterfly over them leaves the row's minimum
    // in every lane; lane (reg) keeps the one of register reg, so that the atomics of a 32-row block go out as one instruction over 256
    // contiguous bytes.
    int rst[2], jj[2];
    float cn[2];
    bool ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + f32_tile_col(j);
        const int cc = col < nd ? col : nd - 1;
        rst[j] = cc / kpad;      // uniform over the 32 lanes: kpad % 32 == 0
        jj[j] = cc - rst[j] * kpad;
        ok[j] = col < nd && jj[j] < k && status[rst[j]] != 2;
        cn[j] = cnorm[cc];
    }
    const bool one_restart = rst[0] == rst[1];      // wave-uniform: both 32-column groups belong to one restart (always when kpad % 64 == 0)
    auto key_of = [&](int j, float a) __attribute__((always_inline)) {
        const float dist = cn[j] - 2.0f * a;
        // not rank_key: the SMALLEST key wins (nearest centre, then lower j), so the index is not inverted and KEY_NONE is all ones
        return ok[j] ? ((unsigned long long)mono32(dist + 0.0f) << 32) | (unsigned long long)(unsigned)jj[j] : KEY_NONE;
    };
    auto row_min = [&](unsigned long long key) __attribute__((always_inline)) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(key, o);
            key = t < key ? t : key;
        }
        return key;
    };
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        unsigned long long mine[2] = {KEY_NONE, KEY_NONE};
        if (one_restart) {      // the two groups are merged in the lane first: half the butterflies (the lower column wins a tie: it has the lower j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned long long a = key_of(0, acc[i][0][r]), b = key_of(1, acc[i][1][r]);
                const unsigned long long key = row_min(b < a ? b : a);
                if ((lane & 31) == r) mine[0] = key;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned long long key = row_min(key_of(j, acc[i][j][r]));
                    if ((lane & 31) == r) mine[j] = key;
                }
        }
        const int reg = lane & 31;
        const int q = q0 + f32_tile_row(i, reg);
        if (reg < 16 && q < nq) {
            if (mine[0] != KEY_NONE) atomicMin(best + (int64_t)rst[0] * nq + q, mine[0]);
            if (!one_restart && mine[1] != KEY_NONE) atomicMin(best + (int64_t)rst[1] * nq + q, mine[1]);
        }
    }
}

__global__ __launch_bounds__(256) void clus_post_kernel(const unsigned long long* __restrict__ best, int n, int k, const int32_t* __restrict__ status,
                                                         int32_t* __restrict__ labels, int32_t* __restrict__ changed) {
    __shared__ long long red[4];
    const int r = blockIdx.y, tid = threadIdx.x;
    if (status[r] == 2) return;
    const int i = blockIdx.x * 256 + tid;
    long long ch = 0;
    if (i < n) {
        const unsigned long long key = best[(int64_t)r * n + i];
        int lab = key == KEY_NONE ? 0 : (int)(unsigned)(key & 0xFFFFFFFFull);
        lab = lab < k ? lab : 0;
        ch = labels[(int64_t)r * n + i] != lab;
        labels[(int64_t)r * n + i] = lab;
    }
    const long long tot = block_reduce<4>(ch, BlockSum(), red);
    if (tid == 0 && tot) atomicAdd(changed + r, (int)tot);
}

// ---------------------------------------------------------------------------------------------------------------------------------
//  Stage 4: update
// ---------------------------------------------------------------------------------------------------------------------------------
// Workgroup (r * k + j, column block): walks restart r's labels 256 at a time, compacts the rows of cluster j in order (ballot + prefix),
// and adds them one after the other: the sum's order is the row order, whatever the machine does.
__global__ __launch_bounds__(256) void clus_update_kernel(const float* __restrict__ xc, int n, int dpad, int k, int kpad, const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ status, float* __restrict__ sums, int32_t* __restrict__ counts) {
    __shared__ int list[2][256];
    __shared__ int wcnt[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = blockIdx.x / k, j = blockIdx.x - r * k;
    if (status[r] != 0) return;
    const int32_t* __restrict__ lab = labels + (int64_t)r * n;
    const int cbase = blockIdx.y * 1024 + tid;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int total = 0;
    for (int base = 0, b = 0; base < n; base += 256, b ^= 1) {
        const int i = base + tid;
        const bool m = i < n && lab[i] == j;
        const unsigned long long bal = __ballot(m);
        if (lane == 0) wcnt[b][wid] = (int)__popcll(bal);
        __syncthreads();
        int off = 0, cnt = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = wcnt[b][w];
            off += w < wid ? c : 0;
            cnt += c;
        }
        if (m) list[b][off + (int)__popcll(bal & ((1ull << lane) - 1ull))] = i;
        __syncthreads();
        int e = 0;
        for (; e + 4 <= cnt; e += 4) {
            float v[4][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float* row = xc + (int64_t)list[b][e + t] * dpad;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[t][q] = cbase + q * 256 < dpad ? row[cbase + q * 256] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = acc[q] + v[t][q];
        }
        for (; e < cnt; ++e) {
            const float* row = xc + (int64_t)list[b][e] * dpad;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = acc[q] + (cbase + q * 256 < dpad ? row[cbase + q * 256] : 0.f);
        }
        total += cnt;
    }
    float* out = sums + ((int64_t)r * kpad + j) * dpad;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (cbase + q * 256 < dpad) out[cbase + q * 256] = acc[q];
    if (blockIdx.y == 0 && tid == 0) counts[r * kpad + j] = total;
}

__global__ __launch_bounds__(1024) void clus_relocate_kernel(const float* __restrict__ xc, const float* __restrict__ xnorm, int n, int dpad, int k, int kpad,
                                                              const int32_t* __restrict__ labels, const int32_t* __restrict__ status,
                                                              unsigned long long* __restrict__ best, float* __restrict__ sums, int32_t* __restrict__ counts) {
    __shared__ unsigned long long red[16];
    __shared__ int empties[CLUS_MAX_K];
    __shared__ int n_empty;
    const int tid = threadIdx.x, r = blockIdx.x;
    if (status[r] != 0) return;
    int32_t* cnt = counts + r * kpad;
    if (tid == 0) {      // the clusters that are empty now, ascending; a donor that runs dry below is not refilled
        int e = 0;
        for (int j = 0; j < k; ++j)
            if (cnt[j] == 0) empties[e++] = j;
        n_empty = e;
    }
    __syncthreads();
    const int ne = n_empty;
    if (ne == 0) return;
    unsigned long long* bk = best + (int64_t)r * n;
    for (int it = 0; it < ne; ++it) {
        // the point farthest from its assigned centre (||x||^2 added back to the assign stage's minimum), lowest index on ties; a point that
        // has moved is marked KEY_NONE and not looked at again
        unsigned long long m = 0ull;
        for (int i = tid; i < n; i += 1024) {
            const unsigned long long key = bk[i];
            if (key == KEY_NONE) continue;
            const float dist = mono32_inv((unsigned)(key >> 32)) + xnorm[i];      // the assign key's high word
            const unsigned long long cand = rank_key(dist + 0.0f, (unsigned)i);
            m = cand > m ? cand : m;
        }
        const unsigned long long top = block_reduce<16>(m, BlockMax(), red);      // red is next written behind the barrier that ends this round
        if (top == 0ull) return;      // block-uniform: no point left
        const int dst = empties[it];
        const int p = (int)rank_key_index(top);
        const int src = labels[(int64_t)r * n + p];
        float* s_src = sums + ((int64_t)r * kpad + src) * dpad;
        float* s_dst = sums + ((int64_t)r * kpad + dst) * dpad;
        const float* row = xc + (int64_t)p * dpad;
        for (int c = tid; c < dpad; c += 1024) {
            const float v = row[c];
            s_src[c] = s_src[c] - v;
            s_dst[c] = v;
        }
        if (tid == 0) {
            cnt[src] -= 1;
            cnt[dst] = 1;
            bk[p] = KEY_NONE;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
//  Stage 5: new centres, shift, stopping rules
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void clus_decide_kernel(int dpad, int k, int kpad, int max_iter, const double* __restrict__ tol_abs,
                                                            const float* __restrict__ sums, const int32_t* __restrict__ counts, float* __restrict__ centres,
                                                            int32_t* __restrict__ status, int32_t* __restrict__ n_iter, int32_t* __restrict__ changed) {
    __shared__ double red[1024];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int st = status[r];
    if (st == 2) return;
    if (st == 1) {      // this iteration's assign was the closing one
        if (tid == 0) {
            status[r] = 2;
            changed[r] = 0;
        }
        return;
    }
    double shift = 0.0;
    const int64_t total = (int64_t)k * dpad;
    for (int64_t e = tid; e < total; e += 1024) {
        const int j = (int)(e / dpad);
        const int64_t at = (int64_t)r * kpad * dpad + e;
        const int c = counts[r * kpad + j];
        float v = sums[at];
        if (c > 0) v = v * (1.0f / (float)c);
        const float df = v - centres[at];
        shift += (double)df * (double)df;
        centres[at] = v;
    }
    const double tot = block_tree_sum<1024>(shift, red);
    if (tid == 0) {
        const int it = n_iter[r] + 1;
        n_iter[r] = it;
        if (changed[r] == 0) status[r] = 2;                              // labels as in the previous iteration: the new centres are kept
        else if (tot <= tol_abs[0] || it >= max_iter) status[r] = 1;     // one more assign, so that the labels match the final centres
        changed[r] = 0;
    }
}

// restarts still running; 0 when the input held a NaN or an infinity (nothing to wait for: the caller reports the flag instead)
__global__ void clus_count_kernel(const int32_t* __restrict__ status, int R, const int32_t* __restrict__ nonfinite, int32_t* __restrict__ unfinished,
                                  int32_t* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int u = 0;
        for (int r = 0; r < R; ++r) u += status[r] != 2;
        if (nonfinite[0]) u = 0;
        unfinished[0] = u;
        if (out) out[0] = u;
    }
}

__global__ __launch_bounds__(256) void clus_set_init_kernel(const float* __restrict__ init, int64_t ld, int k, int d, int dpad, const float* __restrict__ mean,
                                                             float* __restrict__ centres) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)k * dpad) return;
    const int j = (int)(e / dpad), c = (int)(e - (int64_t)j * dpad);
    centres[e] = c < d ? init[(int64_t)j * ld + c] - mean[c] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
//  Stage 6: inertia, selection, export
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clus_inertia_kernel(const float* __restrict__ xc, int n, int dpad, int kpad, const int32_t* __restrict__ labels,
                                                            const float* __restrict__ centres, double* __restrict__ ipart) {
    __shared__ double red[256];
    const int tid = threadIdx.x, r = blockIdx.y;
    const int i = blockIdx.x * 256 + tid;
    float s = 0.f;
    if (i < n) {
        int lab = labels[(int64_t)r * n + i];
        lab = lab < 0 ? 0 : lab;
        const f32x4* x = (const f32x4*)(xc + (int64_t)i * dpad);
        const f32x4* c = (const f32x4*)(centres + ((int64_t)r * kpad + lab) * dpad);
        for (int q = 0; q < dpad / 4; ++q) {
            const f32x4 a = x[q], b = c[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float df = a[e] - b[e];
                s = s + df * df;
            }
        }
    }
    const double tot = block_tree_sum<256>((double)s, red);
    if (tid == 0) ipart[(int64_t)r * gridDim.x + blockIdx.x] = tot;
}

// summary: [0] winning restart, [1] its n_iter, [2] 1 = every input value finite, [3] restarts not finished
__global__ void clus_select_kernel(const double* __restrict__ ipart, int nblk, int R, const int32_t* __restrict__ n_iter, const int32_t* __restrict__ nonfinite,
                                   const int32_t* __restrict__ status, double* __restrict__ inertia, int32_t* __restrict__ summary) {
    __shared__ double tot[CLUS_MAX_INIT];
    const int r = threadIdx.x;
    if (r < R) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += ipart[(int64_t)r * nblk + b];
        tot[r] = s;
        inertia[r] = s;
    }
    __syncthreads();
    if (r == 0) {
        int best = 0, u = 0;
        for (int q = 1; q < R; ++q)
            if (tot[q] < tot[best]) best = q;
        for (int q = 0; q < R; ++q) u += status[q] != 2;
        summary[0] = best;
        summary[1] = n_iter[best];
        summary[2] = nonfinite[0] == 0;
        summary[3] = u;
    }
}

__global__ __launch_bounds__(256) void clus_export_kernel(const int32_t* __restrict__ summary, int n, int d, int dpad, int k, int kpad,
                                                           const int32_t* __restrict__ labels, const float* __restrict__ centres, const float* __restrict__ mean,
                                                           int32_t* __restrict__ labels_out, float* __restrict__ centres_out) {
    const int best = summary[0];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) labels_out[e] = labels[(int64_t)best * n + e];
    if (e < (int64_t)k * d) {
        const int j = (int)(e / d), c = (int)(e - (int64_t)j * d);
        centres_out[e] = centres[((int64_t)best * kpad + j) * dpad + c] + mean[c];
    }
}

__global__ __launch_bounds__(256) void clus_copy_i32_kernel(const int32_t* __restrict__ src, int64_t n, int32_t* __restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = src[e];
}

// ---------------------------------------------------------------------------------------------------------------------------------
//  Stage 7: scores
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clus_contingency_kernel(const int32_t* __restrict__ a, int na, const int32_t* __restrict__ b, int nb, int n,
                                                                int32_t* __restrict__ table) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = a[i], y = b[i];
    if (x < 0 || x >= na || y < 0 || y >= nb) return;      // ids are dense by contract; anything else is left out instead of written somewhere
    atomicAdd(table + (int64_t)x * nb + y, 1);
}

// table [na, nb] -> out[0..2] = ARI, NMI (arithmetic mean of the entropies), V-measure (beta = 1); marg = scratch of na + nb int64.
// scikit-learn's formulas: adjusted_rand_score from the pair confusion matrix, mutual_info_score term by term over the non-zero cells,
// entropy over the non-empty classes, homogeneity_completeness_v_measure.
__global__ __launch_bounds__(256) void clus_scores_kernel(const int32_t* __restrict__ table, int na, int nb, long long* __restrict__ marg,
                                                           double* __restrict__ out) {
    __shared__ double redd[256];
    __shared__ long long redi[6][4];      // block_reduce has no trailing barrier: the six sums take a row each
    const int tid = threadIdx.x;
    long long* ra = marg;
    long long* cb = marg + na;
    for (int i = tid; i < na; i += 256) {
        long long s = 0;
        for (int j = 0; j < nb; ++j) s += table[(int64_t)i * nb + j];
        ra[i] = s;
    }
    for (int j = tid; j < nb; j += 256) {
        long long s = 0;
        for (int i = 0; i < na; ++i) s += table[(int64_t)i * nb + j];
        cb[j] = s;
    }
    __threadfence_block();
    __syncthreads();
    long long ss = 0, sa = 0, sb = 0, nn = 0, ca = 0, cbn = 0;
    for (int64_t e = tid; e < (int64_t)na * nb; e += 256) {
        const long long v = table[e];
        ss += v * v;
    }
    for (int i = tid; i < na; i += 256) {
        sa += ra[i] * ra[i];
        nn += ra[i];
        ca += ra[i] > 0;
    }
    for (int j = tid; j < nb; j += 256) {
        sb += cb[j] * cb[j];
        cbn += cb[j] > 0;
    }
    ss = block_reduce<4>(ss, BlockSum(), redi[0]);
    sa = block_reduce<4>(sa, BlockSum(), redi[1]);
    sb = block_reduce<4>(sb, BlockSum(), redi[2]);
    nn = block_reduce<4>(nn, BlockSum(), redi[3]);
    ca = block_reduce<4>(ca, BlockSum(), redi[4]);
    cbn = block_reduce<4>(cbn, BlockSum(), redi[5]);
    const double N = (double)nn, logN = log(N);
    // entropies and mutual information
    double ha = 0.0, hb = 0.0, mi = 0.0;
    for (int i = tid; i < na; i += 256)
        if (ra[i] > 0) ha += ((double)ra[i] / N) * (log((double)ra[i]) - logN);
    for (int j = tid; j < nb; j += 256)
        if (cb[j] > 0) hb += ((double)cb[j] / N) * (log((double)cb[j]) - logN);
    if (ca > 1 && cbn > 1)
        for (int64_t e = tid; e < (int64_t)na * nb; e += 256) {
            const long long v = table[e];
            if (v > 0) {
                const int i = (int)(e / nb), j = (int)(e - (int64_t)i * nb);
                const double nm = (double)v / N;
                const double log_outer = -log((double)(ra[i] * cb[j])) + logN + logN;
                const double t = nm * (log((double)v) - logN) + nm * log_outer;
                mi += fabs(t) < 2.220446049250313e-16 ? 0.0 : t;
            }
        }
    ha = -block_tree_sum<256>(ha, redd);
    hb = -block_tree_sum<256>(hb, redd);
    mi = block_tree_sum<256>(mi, redd);
    if (tid != 0) return;
    if (ca <= 1) ha = 0.0;
    if (cbn <= 1) hb = 0.0;
    mi = mi < 0.0 ? 0.0 : mi;
    // ARI
    const long long tp = ss - nn, fp = sb - ss, fn = sa - ss, tn = nn * nn - fp - fn - ss;
    double ari = 1.0;
    if (!(fn == 0 && fp == 0))
        ari = 2.0 * ((double)tp * (double)tn - (double)fn * (double)fp) /
              (((double)tp + (double)fn) * ((double)fn + (double)tn) + ((double)tp + (double)fp) * ((double)fp + (double)tn));
    // NMI
    double nmi;
    if (ca == 1 && cbn == 1) nmi = 1.0;
    else if (mi == 0.0) nmi = 0.0;
    else nmi = mi / ((ha + hb) * 0.5);
    // V-measure
    const double hom = ha != 0.0 ? mi / ha : 1.0;
    const double com = hb != 0.0 ? mi / hb : 1.0;
    const double vm = hom + com == 0.0 ? 0.0 : 2.0 * hom * com / (hom + com);
    out[0] = ari;
    out[1] = nmi;
    out[2] = vm;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct Workspace {
    float *xc, *xnorm, *mean;
    double *colpart, *tol_abs;
    int32_t* nonfinite;
    float *centres, *sums, *cnorm;
    unsigned long long* best;
    int32_t* labels;
    float *closest, *mind;
    double* cum;
    int32_t *cand, *cand2, *seeds, *counts, *changed, *status, *n_iter, *unfinished;
    double *inertia, *ipart;
    size_t bytes;
};

static Workspace carve(void* ws, int64_t n, int d, int k, int R) {
    Workspace w;
    const size_t dp = (size_t)dpad_of(d), kp = (size_t)kpad_of(k), T = (size_t)trials_of(k);
    char* p = (char*)ws;
    // the part that depends on (n, d) only comes first: one prepared workspace serves every k up to the one it was sized for
    w.xc = take<float>(p, (size_t)n * dp);
    w.xnorm = take<float>(p, (size_t)n);
    w.mean = take<float>(p, dp);
    w.colpart = take<double>(p, (size_t)NCHUNK * dp);
    w.tol_abs = take<double>(p, 1);
    w.nonfinite = take<int32_t>(p, 1);
    w.centres = take<float>(p, (size_t)R * kp * dp);
    w.sums = take<float>(p, (size_t)R * kp * dp);
    w.cnorm = take<float>(p, (size_t)R * kp);
    w.best = take<unsigned long long>(p, (size_t)R * n);
    w.labels = take<int32_t>(p, (size_t)R * n);
    w.closest = take<float>(p, (size_t)R * n);
    w.mind = take<float>(p, (size_t)R * T * n);
    w.cum = take<double>(p, (size_t)R * n);
    w.cand = take<int32_t>(p, (size_t)R * T);
    w.cand2 = take<int32_t>(p, (size_t)R * T);
    w.seeds = take<int32_t>(p, (size_t)R * k);
    w.counts = take<int32_t>(p, (size_t)R * kp);
    w.changed = take<int32_t>(p, (size_t)R);
    w.status = take<int32_t>(p, (size_t)R);
    w.n_iter = take<int32_t>(p, (size_t)R);
    w.unfinished = take<int32_t>(p, 1);
    w.inertia = take<double>(p, (size_t)R);
    w.ipart = take<double>(p, (size_t)R * (size_t)((n + 255) / 256));
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

static int check_args(const avexhip_clustering_args* a, const char* what, Workspace* w) {
    AVX_REQUIRE(a && a->workspace, "%s: null argument", what);
    AVX_REQUIRE(a->n >= 1 && a->n <= CLUS_MAX_N && a->d >= 1, "%s: bad shape (n %d [1, %d], d %d)", what, a->n, CLUS_MAX_N, a->d);
    AVX_REQUIRE(a->k >= 1 && a->k <= CLUS_MAX_K && a->k <= a->n, "%s: k %d outside [1, min(n, %d)]", what, a->k, CLUS_MAX_K);
    AVX_REQUIRE(a->n_init >= 1 && a->n_init <= CLUS_MAX_INIT, "%s: n_init %d outside [1, %d]", what, a->n_init, CLUS_MAX_INIT);
    AVX_REQUIRE((int64_t)a->n_init * kpad_of(a->k) * dpad_of(a->d) < ((int64_t)1 << 40), "%s: centre table too large", what);
    *w = carve(a->workspace, a->n, a->d, a->k, a->n_init);
    if (a->workspace_bytes < w->bytes) {
        avexhip_set_error("%s: workspace %zu B < %zu B", what, a->workspace_bytes, w->bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    return AVEXHIP_OK;
}

static int reset_state(const avexhip_clustering_args* a, const Workspace& w, hipStream_t s) {
    const size_t dp = (size_t)dpad_of(a->d), kp = (size_t)kpad_of(a->k);
    const int R = a->n_init;
    AVX_HIP_CHECK(hipMemsetAsync(w.centres, 0, (size_t)R * kp * dp * 4, s));      // pad rows and pad columns stay zero
    AVX_HIP_CHECK(hipMemsetAsync(w.sums, 0, (size_t)R * kp * dp * 4, s));
    AVX_HIP_CHECK(hipMemsetAsync(w.labels, 0xFF, (size_t)R * a->n * 4, s));         // -1: the first iteration changes every label
    AVX_HIP_CHECK(hipMemsetAsync(w.counts, 0, (size_t)R * kp * 4, s));
    AVX_HIP_CHECK(hipMemsetAsync(w.changed, 0, (size_t)R * 4, s));
    AVX_HIP_CHECK(hipMemsetAsync(w.status, 0, (size_t)R * 4, s));
    AVX_HIP_CHECK(hipMemsetAsync(w.n_iter, 0, (size_t)R * 4, s));
    AVX_HIP_CHECK(hipMemsetAsync(w.seeds, 0xFF, (size_t)R * a->k * 4, s));
    return AVEXHIP_OK;
}

}  // namespace

extern "C" size_t avexhip_clustering_workspace_bytes(int64_t n, int d, int k, int n_init) {
    if (n <= 0 || n > CLUS_MAX_N || d <= 0 || k <= 0 || k > CLUS_MAX_K || n_init <= 0 || n_init > CLUS_MAX_INIT) return 0;
    return carve(nullptr, n, d, k, n_init).bytes;
}

extern "C" int avexhip_clustering_max_k(void) { return CLUS_MAX_K; }

extern "C" const float* avexhip_clustering_centred_rows(const avexhip_clustering_args* a) {
    if (!a || !a->workspace || a->n < 1 || a->n > CLUS_MAX_N || a->d < 1 || a->k < 1 || a->k > CLUS_MAX_K || a->n_init < 1 || a->n_init > CLUS_MAX_INIT) return nullptr;
    const Workspace w = carve(a->workspace, a->n, a->d, a->k, a->n_init);
    return a->workspace_bytes >= w.bytes ? w.xc : nullptr;
}

extern "C" int avexhip_clustering_trials(int k) { return k >= 1 ? trials_of(k) : 0; }

extern "C" int avexhip_clustering_prepare(const avexhip_clustering_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "clustering_prepare", &w));
    AVX_REQUIRE(a->x && a->ld_x >= a->d, "clustering_prepare: embeddings missing");
    hipStream_t s = (hipStream_t)stream;
    const int dp = (int)dpad_of(a->d);
    const int rows_per = (a->n + NCHUNK - 1) / NCHUNK;
    const dim3 grid(NCHUNK, (dp + 255) / 256);
    AVX_HIP_CHECK(hipMemsetAsync(w.nonfinite, 0, 4, s));
    clus_colsum_kernel<<<grid, dim3(256), 0, s>>>(a->x, a->ld_x, a->n, a->d, dp, rows_per, w.colpart, w.nonfinite);
    AVX_LAUNCH_CHECK();
    clus_mean_kernel<<<dim3((dp + 255) / 256), dim3(256), 0, s>>>(w.colpart, a->n, a->d, dp, w.mean);
    AVX_LAUNCH_CHECK();
    clus_centre_kernel<<<grid, dim3(256), 0, s>>>(a->x, a->ld_x, a->n, a->d, dp, rows_per, w.mean, w.xc, w.colpart);
    AVX_LAUNCH_CHECK();
    clus_tol_kernel<<<dim3(1), dim3(256), 0, s>>>(w.colpart, a->n, a->d, dp, (double)a->tol, w.tol_abs);
    AVX_LAUNCH_CHECK();
    clus_rownorm_kernel<<<dim3((a->n + 255) / 256), dim3(256), 0, s>>>(w.xc, a->n, dp, w.xnorm);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_clustering_seed(const avexhip_clustering_args* a, const int32_t* first_dev, const double* u_dev, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "clustering_seed", &w));
    AVX_REQUIRE(first_dev && (u_dev || a->k == 1), "clustering_seed: draws missing");
    hipStream_t s = (hipStream_t)stream;
    AVXH_TRY(reset_state(a, w, s));
    const int dp = (int)dpad_of(a->d), kp = kpad_of(a->k), R = a->n_init, T = trials_of(a->k), n = a->n;
    const int nblk = (n + 255) / 256;
    int32_t *cand = w.cand, *next = w.cand2;
    clus_copy_i32_kernel<<<dim3(1), dim3(256), 0, s>>>(first_dev, R, cand);
    AVX_LAUNCH_CHECK();
    for (int c = 0; c < a->k; ++c) {
        const int T_in = c == 0 ? 1 : T;
        const int n_cand = R * T_in;
        clus_seed_dist_kernel<<<dim3(nblk, (n_cand + SG - 1) / SG), dim3(256), 0, s>>>(w.xc, n, dp, cand, n_cand, T_in, c == 0, w.closest, w.mind);
        AVX_LAUNCH_CHECK();
        clus_seed_pick_kernel<<<dim3(R), dim3(1024), 0, s>>>(w.xc, n, dp, a->k, kp, c, T_in, T, u_dev, w.mind, w.closest, w.cum, cand, next, w.seeds,
                                                              w.centres);
        AVX_LAUNCH_CHECK();
        int32_t* t = cand;
        cand = next;
        next = t;
    }
    return AVEXHIP_OK;
}

extern "C" int avexhip_clustering_set_init(const avexhip_clustering_args* a, const float* init_dev, int64_t ld_init, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "clustering_set_init", &w));
    AVX_REQUIRE(init_dev && ld_init >= a->d && a->n_init == 1, "clustering_set_init: one run from [k, d] centres (n_init %d)", a->n_init);
    hipStream_t s = (hipStream_t)stream;
    AVXH_TRY(reset_state(a, w, s));
    const int dp = (int)dpad_of(a->d);
    const int64_t total = (int64_t)a->k * dp;
    clus_set_init_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(init_dev, ld_init, a->k, a->d, dp, w.mean, w.centres);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_clustering_iterate(const avexhip_clustering_args* a, int n_iters, int stages, int32_t* unfinished_out_dev, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "clustering_iterate", &w));
    AVX_REQUIRE(n_iters >= 1 && a->max_iter >= 1, "clustering_iterate: n_iters %d, max_iter %d", n_iters, a->max_iter);
    hipStream_t s = (hipStream_t)stream;
    const int dp = (int)dpad_of(a->d), kp = kpad_of(a->k), R = a->n_init, n = a->n, k = a->k;
    const int st = stages == 0 ? 3 : stages;
    AVX_ENSURE_LDS(clus_assign_kernel, FT_LDS_BYTES);
    for (int it = 0; it < n_iters; ++it) {
        if (st & 1) {
            clus_cnorm_kernel<<<dim3((R * kp + 255) / 256), dim3(256), 0, s>>>(w.centres, R * kp, dp, w.cnorm);
            AVX_LAUNCH_CHECK();
            AVX_HIP_CHECK(hipMemsetAsync(w.best, 0xFF, (size_t)R * n * 8, s));
            clus_assign_kernel<<<dim3((R * kp + FT_BN - 1) / FT_BN, (n + FT_BM - 1) / FT_BM), dim3(256), FT_LDS_BYTES, s>>>(w.xc, n, w.centres, R * kp, dp, k, kp,
                                                                                                                    w.cnorm, w.status, w.best);
            AVX_LAUNCH_CHECK();
        }
        if (st & 2) {
            clus_post_kernel<<<dim3((n + 255) / 256, R), dim3(256), 0, s>>>(w.best, n, k, w.status, w.labels, w.changed);
            AVX_LAUNCH_CHECK();
            clus_update_kernel<<<dim3(R * k, (dp + 1023) / 1024), dim3(256), 0, s>>>(w.xc, n, dp, k, kp, w.labels, w.status, w.sums, w.counts);
            AVX_LAUNCH_CHECK();
            clus_relocate_kernel<<<dim3(R), dim3(1024), 0, s>>>(w.xc, w.xnorm, n, dp, k, kp, w.labels, w.status, w.best, w.sums, w.counts);
            AVX_LAUNCH_CHECK();
            clus_decide_kernel<<<dim3(R), dim3(1024), 0, s>>>(dp, k, kp, a->max_iter, w.tol_abs, w.sums, w.counts, w.centres, w.status, w.n_iter, w.changed);
            AVX_LAUNCH_CHECK();
        }
    }
    clus_count_kernel<<<dim3(1), dim3(64), 0, s>>>(w.status, R, w.nonfinite, w.unfinished, unfinished_out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_clustering_finish(const avexhip_clustering_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "clustering_finish", &w));
    AVX_REQUIRE(a->labels_out && a->centers_out && a->inertias_out && a->n_iters_out && a->seeds_out && a->summary_out, "clustering_finish: null output");
    hipStream_t s = (hipStream_t)stream;
    const int dp = (int)dpad_of(a->d), kp = kpad_of(a->k), R = a->n_init, n = a->n, k = a->k;
    const int nblk = (n + 255) / 256;
    clus_inertia_kernel<<<dim3(nblk, R), dim3(256), 0, s>>>(w.xc, n, dp, kp, w.labels, w.centres, w.ipart);
    AVX_LAUNCH_CHECK();
    clus_select_kernel<<<dim3(1), dim3(CLUS_MAX_INIT), 0, s>>>(w.ipart, nblk, R, w.n_iter, w.nonfinite, w.status, a->inertias_out, a->summary_out);
    AVX_LAUNCH_CHECK();
    const int64_t total = (int64_t)k * a->d > n ? (int64_t)k * a->d : n;
    clus_export_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(a->summary_out, n, a->d, dp, k, kp, w.labels, w.centres, w.mean,
                                                                                a->labels_out, a->centers_out);
    AVX_LAUNCH_CHECK();
    clus_copy_i32_kernel<<<dim3(1), dim3(256), 0, s>>>(w.n_iter, R, a->n_iters_out);
    AVX_LAUNCH_CHECK();
    clus_copy_i32_kernel<<<dim3((unsigned)(((int64_t)R * k + 255) / 256)), dim3(256), 0, s>>>(w.seeds, (int64_t)R * k, a->seeds_out);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" size_t avexhip_clustering_scores_workspace_bytes(int n_true, int n_pred) {
    if (n_true <= 0 || n_pred <= 0) return 0;
    return align256((size_t)n_true * n_pred * 4) + align256(((size_t)n_true + n_pred) * 8);
}

extern "C" int avexhip_clustering_scores(const int32_t* true_ids_dev, int n_true, const int32_t* pred_ids_dev, int n_pred, int n, void* workspace,
                                         size_t workspace_bytes, double* out_dev, void* stream) {
    AVX_REQUIRE(true_ids_dev && pred_ids_dev && workspace && out_dev, "clustering_scores: null argument");
    AVX_REQUIRE(n >= 1 && n_true >= 1 && n_pred >= 1 && (int64_t)n_true * n_pred <= ((int64_t)1 << 28), "clustering_scores: bad shape (n %d, %d x %d)", n,
                n_true, n_pred);
    const size_t need = avexhip_clustering_scores_workspace_bytes(n_true, n_pred);
    if (workspace_bytes < need) {
        avexhip_set_error("clustering_scores: workspace %zu B < %zu B", workspace_bytes, need);
        return AVEXHIP_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    int32_t* table = (int32_t*)workspace;
    long long* marg = (long long*)((char*)workspace + align256((size_t)n_true * n_pred * 4));
    AVX_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)n_true * n_pred * 4, s));
    clus_contingency_kernel<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(true_ids_dev, n_true, pred_ids_dev, n_pred, n, table);
    AVX_LAUNCH_CHECK();
    clus_scores_kernel<<<dim3(1), dim3(256), 0, s>>>(table, n_true, n_pred, marg, out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
