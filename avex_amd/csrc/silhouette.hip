// Silhouette coefficient on the device: scikit-learn's silhouette_samples / silhouette_score (metric "euclidean" or "cosine") for embeddings
// that already live in HBM.  O(N^2 D) pairwise distances on the fp32 MFMA tile of f32_tile.h, reduced per (point, cluster) in the epilogue;
// the N x N matrix is never written.
//
// Layout: the caller orders the rows by cluster, every cluster padded to a multiple of 32 slots and the whole to a multiple of 128
// (slot_src[slot] = input row or -1, group_label[slot / 32] = cluster or -1).  A 32-column group of a tile then belongs to one cluster.
//
//   sil_gather_kernel     slot -> row of the working matrix (width padded to the K tile): the input row as it is ("euclidean": the caller
//                         passes centred rows) or divided by max(||row||, 1e-12) ("cosine", the arithmetic of retr_normalize_kernel); padding
//                         slots are zero rows; the finite flag
//   sil_diag_kernel       ||row||^2 as the DIAGONAL of the same tile product that gives the Gram entries: two bit-identical rows x, y then have
//                         x.x == y.y == x.y bit for bit and (||x||^2 + ||y||^2) - 2 x.y == 0 exactly.  -1 marks a padding slot.  The largest
//                         norm (integer atomicMax on the float's bits) fixes the fixed-point scale below.
//   sil_scale_kernel      scale = 2^e with n_slots * (largest possible distance) * scale < 2^62
//   sil_dist_kernel       workgroup (column segment, 128-row tile): for each 128-column tile of its segment the product, then
//                         d = sqrt(max((||x||^2 + ||y||^2) - 2 x.y, 0)) or clip(1 - x.y, 0, 2), 0 on the diagonal and for padding columns, written
//                         to LDS (the operand buffers are free by then); thread (row, 32-column group) adds its 32 distances in ascending column
//                         order in fp64, rounds the sum ONCE to 64-bit fixed point and keeps an integer running sum while the group's cluster
//                         stays the same; on a change it goes out with one 64-bit INTEGER atomicAdd to sums[cluster][row].  Integer addition is
//                         associative: the result does not depend on the order of the atomics, on the segment length or on the batch.
//   sil_samples_kernel    per point, fp64: a = own sum / (size - 1), b = min over the other clusters of sum / size, s = (b - a) / max(a, b);
//                         0 for a cluster of one and for 0 / 0 (sklearn's nan_to_num)
//   sil_mean_kernel       fp64 mean of the samples in a fixed order, and the finite flag
//
// The symmetry of the distance matrix is not used: every pair is computed twice.
// Limits: n <= 524288, n_labels <= 4096.
#include "block_prims.h"
#include "f32_tile.h"

namespace {

constexpr int SIL_MAX_N = 1 << 19, SIL_MAX_LABELS = 4096;
constexpr int SIL_LDD = FT_BN + 4;                                 // floats per row of the distance tile in LDS: rows 528 B apart, so that
                                                                   // 16 threads reading 16 B of 16 consecutive rows hit 16 different bank quads
constexpr int SIL_LDS_BYTES = FT_BM * SIL_LDD * 4;                 // 67 584 B >= FT_LDS_BYTES
static_assert(SIL_LDS_BYTES >= FT_LDS_BYTES, "the distance tile reuses the operand buffers");

struct Workspace {
    float *xs, *nrm;
    unsigned long long* sums;
    double* scale;              // [0] scale, [1] 1 / scale
    unsigned* maxbits;
    int32_t* nonfinite;
    size_t bytes;
};

static Workspace carve(void* ws, int64_t n_slots, int d, int n_labels, int batch) {
    Workspace w;
    char* p = (char*)ws;
    w.xs = take<float>(p, (size_t)n_slots * (size_t)dpad_of(d));
    w.nrm = take<float>(p, (size_t)n_slots);
    w.sums = take<unsigned long long>(p, (size_t)n_labels * (size_t)batch);
    w.scale = take<double>(p, 2);
    w.maxbits = take<unsigned>(p, 1);
    w.nonfinite = take<int32_t>(p, 1);
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

// One wave per slot.
__global__ __launch_bounds__(256) void sil_gather_kernel(const float* __restrict__ x, int64_t ldx, int n, int d, int dpad, int n_slots, int cosine,
                                                          const int32_t* __restrict__ slot_src, float* __restrict__ xs, int32_t* __restrict__ nonfinite) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= n_slots) return;
    float* o = xs + (int64_t)slot * dpad;
    const int src = slot_src[slot];
    if (src < 0 || src >= n) {
        for (int c = lane; c < dpad; c += 64) o[c] = 0.f;
        return;
    }
    const float* r = x + (int64_t)src * ldx;
    bool bad = false;
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float v = r[c];
        bad |= !(__builtin_fabsf(v) <= 3.4028234663852886e38f);
        ss = __builtin_fmaf(v, v, ss);
    }
    float nrm = 1.f;
    if (cosine) {
        nrm = __builtin_sqrtf(wave_sum(ss));
        nrm = nrm < 1e-12f ? 1e-12f : nrm;
    }
    for (int c = lane; c < dpad; c += 64) o[c] = c < d ? (cosine ? r[c] / nrm : r[c]) : 0.f;
    if (bad) atomicOr(nonfinite, 1);
}

__global__ __launch_bounds__(256) void sil_diag_kernel(const float* __restrict__ xs, int n_slots, int dpad, const int32_t* __restrict__ slot_src,
                                                        float* __restrict__ nrm, unsigned* __restrict__ maxbits) {
    const int r0 = blockIdx.x * FT_BM;
    f32x16 acc[2][2];
    f32_tile_product(xs, n_slots, r0, xs, n_slots, r0, dpad, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = f32_tile_col(j);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (f32_tile_row(i, r) == col && r0 + col < n_slots) {
                    const bool real = slot_src[r0 + col] >= 0;
                    const float v = acc[i][j][r];
                    nrm[r0 + col] = real ? v : -1.f;
                    if (real && v > 0.f) atomicMax(maxbits, __float_as_uint(v));      // positive floats order as their bits
                }
        }
}

// The largest distance is at most 2 sqrt(max ||x||^2) < 2^(ceil((E + 1) / 2) + 1) with E the exponent of the largest squared norm (cosine: 2).
__global__ void sil_scale_kernel(const unsigned* __restrict__ maxbits, int n_slots, int cosine, double* __restrict__ scale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int dexp = 1;
    if (!cosine) {
        const int e = (int)((maxbits[0] >> 23) & 0xFFu) - 127;
        const int e1 = e + 1;
        dexp = (e1 >= 0 ? (e1 + 1) / 2 : -((-e1) / 2)) + 1;
    }
    int nexp = 0;
    while (((int64_t)1 << nexp) < n_slots) ++nexp;
    const int se = 62 - nexp - dexp;
    scale[0] = ldexp(1.0, se);
    scale[1] = ldexp(1.0, -se);
}

// sums[cluster * batch + (slot - row0)] += the distances from slot to the members of cluster, over this workgroup's column tiles.
__global__ __launch_bounds__(256) void sil_dist_kernel(const float* __restrict__ xs, int n_slots, int dpad, const float* __restrict__ nrm,
                                                        const int32_t* __restrict__ group_label, int n_labels, int cosine, int row0, int nb,
                                                        int batch, int tiles_per_seg, const double* __restrict__ scale, unsigned long long* __restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dist = (float*)smem;
    const int tid = threadIdx.x;
    const int r0 = row0 + blockIdx.y * FT_BM;
    const int n_tiles = n_slots / FT_BN;
    const int t0 = blockIdx.x * tiles_per_seg;
    const int t1 = t0 + tiles_per_seg < n_tiles ? t0 + tiles_per_seg : n_tiles;
    float rn[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + f32_tile_row(i, r);
            rn[i][r] = row < n_slots ? nrm[row] : -1.f;
        }
    // the reducing role of this thread: row rrow of the tile, column groups g0 and g0 + 2 (a wave has one g0: the branches below are uniform)
    const int rrow = tid & 127, g0 = tid >> 7;
    const int myslot = r0 + rrow;
    const bool mine = myslot < row0 + nb && myslot < n_slots && nrm[myslot] >= 0.f;
    const double sc = scale[0];
    long long run[2] = {0, 0};
    int cur[2] = {-1, -1};
    auto flush = [&](int q) __attribute__((always_inline)) {
        if (cur[q] >= 0 && mine && run[q] != 0) atomicAdd(sums + (int64_t)cur[q] * batch + (myslot - row0), (unsigned long long)run[q]);
    };
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * FT_BN;
        f32x16 acc[2][2];
        f32_tile_product(xs, n_slots, r0, xs, n_slots, c0, dpad, acc);
        __syncthreads();      // every wave has read its last operand tile: the buffers become the distance tile
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = f32_tile_col(j);
            const float cn = nrm[c0 + lc];      // c0 + lc < n_slots: n_slots is a multiple of the tile
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lr = f32_tile_row(i, r);
                    const float g = acc[i][j][r];
                    float dv;
                    if (cosine) {
                        dv = 1.0f - g;
                        dv = dv < 0.f ? 0.f : (dv > 2.f ? 2.f : dv);
                    } else {
                        const float d2 = (rn[i][r] + cn) - 2.0f * g;
                        dv = __builtin_amdgcn_sqrtf(d2 > 0.f ? d2 : 0.f);
                    }
                    if (cn < 0.f || r0 + lr == c0 + lc) dv = 0.f;
                    dist[lr * SIL_LDD + lc] = dv;
                }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int g = g0 + 2 * q;
            int cl = group_label[(c0 >> 5) + g];
            cl = cl < n_labels ? cl : -1;      // never an index outside sums, whatever the caller's table holds
            if (cl != cur[q]) {
                flush(q);
                cur[q] = cl;
                run[q] = 0;
            }
            if (cl >= 0) {
                const f32x4* p = (const f32x4*)(dist + rrow * SIL_LDD + g * 32);
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const f32x4 v = p[c];
#pragma unroll
                    for (int e = 0; e < 4; ++e) s += (double)v[e];
                }
                run[q] += __double2ll_rn(s * sc);
            }
        }
        __syncthreads();      // the next product stages its operands over the distance tile
    }
    flush(0);
    flush(1);
}

__global__ __launch_bounds__(256) void sil_samples_kernel(const unsigned long long* __restrict__ sums, const int32_t* __restrict__ slot_src,
                                                           const int32_t* __restrict__ group_label, const int32_t* __restrict__ counts, int n, int n_labels,
                                                           int row0, int nb, int batch, const double* __restrict__ scale, double* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const int slot = row0 + b;
    const int src = slot_src[slot];
    if (src < 0 || src >= n) return;
    const int own = group_label[slot >> 5];
    const double inv = scale[1];
    double a = 0.0, bmin = __builtin_inf();
    for (int cl = 0; cl < n_labels; ++cl) {
        const int c = counts[cl];
        const double v = (double)(long long)sums[(int64_t)cl * batch + b] * inv;
        if (cl == own) a = c > 1 ? v / (double)(c - 1) : 0.0;
        else if (c > 0) {
            const double m = v / (double)c;
            bmin = m < bmin ? m : bmin;
        }
    }
    double s = 0.0;
    if (own >= 0 && own < n_labels && counts[own] > 1) {
        const double den = a > bmin ? a : bmin;
        s = den > 0.0 && den < __builtin_inf() ? (bmin - a) / den : 0.0;
    }
    out[src] = s;
}

// summary[0] = mean of the samples (thread t adds elements t, t + 256, ...; then a tree), summary[1] = 1 when every input value was finite
__global__ __launch_bounds__(256) void sil_mean_kernel(const double* __restrict__ samples, int n, const int32_t* __restrict__ nonfinite,
                                                        double* __restrict__ summary) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += samples[i];
    const double tot = block_tree_sum<256>(s, red);
    if (tid == 0) {
        summary[0] = tot / (double)n;
        summary[1] = nonfinite[0] == 0 ? 1.0 : 0.0;
    }
}

static int check_args(const avexhip_silhouette_args* a, const char* what, Workspace* w) {
    AVX_REQUIRE(a && a->workspace && a->slot_src && a->group_label && a->counts, "%s: null argument", what);
    AVX_REQUIRE(a->n >= 2 && a->n <= SIL_MAX_N && a->d >= 1, "%s: bad shape (n %d [2, %d], d %d)", what, a->n, SIL_MAX_N, a->d);
    AVX_REQUIRE(a->n_labels >= 1 && a->n_labels <= SIL_MAX_LABELS, "%s: n_labels %d outside [1, %d]", what, a->n_labels, SIL_MAX_LABELS);
    AVX_REQUIRE(a->n_slots >= a->n && a->n_slots % FT_BN == 0 && (int64_t)a->n_slots <= (int64_t)a->n + 32 * (int64_t)a->n_labels + FT_BN,
                "%s: n_slots %d is not a multiple of %d in [n, n + 32 n_labels + %d]", what, a->n_slots, FT_BN, FT_BN);
    AVX_REQUIRE(a->batch >= 1 && a->batch <= a->n_slots, "%s: batch %d outside [1, n_slots]", what, a->batch);
    AVX_REQUIRE(a->metric == AVEXHIP_SILHOUETTE_EUCLIDEAN || a->metric == AVEXHIP_SILHOUETTE_COSINE, "%s: metric %d", what, a->metric);
    *w = carve(a->workspace, a->n_slots, a->d, a->n_labels, a->batch);
    if (a->workspace_bytes < w->bytes) {
        avexhip_set_error("%s: workspace %zu B < %zu B", what, a->workspace_bytes, w->bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    return AVEXHIP_OK;
}

}  // namespace

extern "C" size_t avexhip_silhouette_workspace_bytes(int64_t n_slots, int d, int n_labels, int batch) {
    if (n_slots <= 0 || n_slots > (int64_t)SIL_MAX_N + 32 * (int64_t)SIL_MAX_LABELS + FT_BN || d <= 0 || n_labels <= 0 || n_labels > SIL_MAX_LABELS ||
        batch <= 0)
        return 0;
    return carve(nullptr, n_slots, d, n_labels, batch).bytes;
}

extern "C" int avexhip_silhouette_max_labels(void) { return SIL_MAX_LABELS; }

extern "C" int avexhip_silhouette_max_n(void) { return SIL_MAX_N; }

extern "C" int avexhip_silhouette_prepare(const avexhip_silhouette_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "silhouette_prepare", &w));
    AVX_REQUIRE(a->x && a->ld_x >= a->d, "silhouette_prepare: rows missing");
    hipStream_t s = (hipStream_t)stream;
    const int dp = (int)dpad_of(a->d);
    const int cosine = a->metric == AVEXHIP_SILHOUETTE_COSINE;
    AVX_HIP_CHECK(hipMemsetAsync(w.nonfinite, 0, 4, s));
    AVX_HIP_CHECK(hipMemsetAsync(w.maxbits, 0, 4, s));
    sil_gather_kernel<<<dim3((a->n_slots + 3) / 4), dim3(256), 0, s>>>(a->x, a->ld_x, a->n, a->d, dp, a->n_slots, cosine, a->slot_src, w.xs, w.nonfinite);
    AVX_LAUNCH_CHECK();
    AVX_ENSURE_LDS(sil_diag_kernel, FT_LDS_BYTES);
    sil_diag_kernel<<<dim3(a->n_slots / FT_BM), dim3(256), FT_LDS_BYTES, s>>>(w.xs, a->n_slots, dp, a->slot_src, w.nrm, w.maxbits);
    AVX_LAUNCH_CHECK();
    sil_scale_kernel<<<dim3(1), dim3(64), 0, s>>>(w.maxbits, a->n_slots, cosine, w.scale);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_silhouette_batch(const avexhip_silhouette_args* a, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "silhouette_batch", &w));
    AVX_REQUIRE(a->samples_out, "silhouette_batch: null output");
    AVX_REQUIRE(a->row0 >= 0 && a->nb >= 1 && a->nb <= a->batch && (int64_t)a->row0 + a->nb <= a->n_slots, "silhouette_batch: slots [%d, +%d) outside [0, %d) or above batch %d",
                a->row0, a->nb, a->n_slots, a->batch);
    hipStream_t s = (hipStream_t)stream;
    const int dp = (int)dpad_of(a->d);
    const int stages = a->stages == 0 ? 3 : a->stages;
    if (stages & 1) {
        const int row_tiles = (a->nb + FT_BM - 1) / FT_BM, n_tiles = a->n_slots / FT_BN;
        int segs = 2048 / row_tiles;      // enough workgroups to fill the chip several times; the result does not depend on this
        segs = segs < 1 ? 1 : (segs > n_tiles ? n_tiles : segs);
        const int per = (n_tiles + segs - 1) / segs;
        AVX_HIP_CHECK(hipMemsetAsync(w.sums, 0, (size_t)a->n_labels * a->batch * 8, s));
        AVX_ENSURE_LDS(sil_dist_kernel, SIL_LDS_BYTES);
        sil_dist_kernel<<<dim3((n_tiles + per - 1) / per, row_tiles), dim3(256), SIL_LDS_BYTES, s>>>(
            w.xs, a->n_slots, dp, w.nrm, a->group_label, a->n_labels, a->metric == AVEXHIP_SILHOUETTE_COSINE, a->row0, a->nb, a->batch, per, w.scale, w.sums);
        AVX_LAUNCH_CHECK();
    }
    if (stages & 2) {
        sil_samples_kernel<<<dim3((a->nb + 255) / 256), dim3(256), 0, s>>>(w.sums, a->slot_src, a->group_label, a->counts, a->n, a->n_labels, a->row0, a->nb,
                                                                        a->batch, w.scale, a->samples_out);
        AVX_LAUNCH_CHECK();
    }
    return AVEXHIP_OK;
}

extern "C" int avexhip_silhouette_finalize(const avexhip_silhouette_args* a, double* summary_out_dev, void* stream) {
    Workspace w;
    AVXH_TRY(check_args(a, "silhouette_finalize", &w));
    AVX_REQUIRE(a->samples_out && summary_out_dev, "silhouette_finalize: null output");
    sil_mean_kernel<<<dim3(1), dim3(256), 0, (hipStream_t)stream>>>(a->samples_out, a->n, w.nonfinite, summary_out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
