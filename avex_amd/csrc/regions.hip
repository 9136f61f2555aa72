// Sound-event regions (ABI 25): the spectrogram cells that stand out of a per-recording threshold spectrum, joined into connected
// regions, one time-frequency box per region -- from the resident waveform of windows.hip and the frames of soundscape.hip.  The
// [frames, 257] spectrogram is never written: 9 words of cell bits per frame are, one integer per frame and nine per set cell.
//   regions_cells_kernel    a run of up to 64 consecutive frames of ONE recording per workgroup; the walk and span staging of
//                           rec_frames.h and wave_frame_power (frame_power.h), the text soundscape_stats_kernel runs: the same P[f, k],
//                           bit for bit; the recording's threshold row in registers, one strict compare per (frame, bin) inside the
//                           band, five wave ballots -> the 9 words of the frame; the recording's non-finite frames by one integer
//                           atomicAdd per wave
//   regions_pack_kernel     the same words from a [frames, 257] mask of bytes (label_cells: a mask from anywhere)
//   prefix_count            (prefix_count.h, shared with density.hip) an exclusive prefix of one small integer per item by counting,
//                           the total in 64 bits.  Used three times: the set cells of each frame (the compact number of a set cell
//                           is offset[f] + popcount(the frame's bits below k), monotone in (recording, frame, bin)), the roots (region
//                           numbers in the order of the smallest cell, no sort), the kept regions (a compaction that keeps order)
//   regions_init_kernel     parent[i] = i; the region accumulators' identities
//   regions_union_kernel    one wave per frame.  A set cell looks at its FORWARD half-neighbourhood inside its recording -- the same
//                           frame at dk = 1 .. rk, the frames f + 1 .. f + rt at dk = -rk .. rk -- in the bit words, and unites itself
//                           with the nearest set cell to its right in its own frame and, in a later frame, with the first cell of every
//                           run of set bits in its window (the rest of a run hangs on that cell through the run's own frame links)
//   regions_flatten_kernel  every cell takes its root
//   regions_boxes_kernel    one wave per frame: the lanes that share a region combine (ballot, butterfly min / max), then ONE integer
//                           atomicAdd (n_cells), atomicMin (low_bin) and two atomicMax (high_bin, last_frame) per (wave, region); the
//                           root cell writes first_frame and recording, which are its own
//   regions_rows_kernel     the kept regions' rows, in order
// Union-find.  unite(a, b) finds both roots and hooks the LARGER under the smaller with atomicMin(parent + larger, smaller); when the
// atomic finds that `larger` had already been hooked elsewhere it goes on with that other parent.  parent[i] <= i always and a word only
// ever decreases (the hooks and the path splitting of rg_find are both atomicMin with a smaller ancestor), so every chain ends at a
// cell that points at itself and every loop ends.  A tree's root is its smallest cell; one tree per component is left when the kernel
// ends, so a region's root is its smallest cell by (recording, frame, bin).  Other threads write parent[k] = (an ancestor of k)
// meanwhile: whichever value a read sees lies on the same chain.  The number of launches does not depend on the mask; no host-polled
// rounds.
// Determinism.  Everything after the compare is integer arithmetic; every atomic is an integer add, min or max on global memory:
// order-free.  Which parent a cell holds between the union and the flatten pass depends on timing, its root does not.  No float atomics.
// Limits: < 2^31 frames, < 2^31 set cells.
#include "block_prims.h"
#include "common.h"
#include "frame_power.h"
#include "prefix_count.h"

namespace {

constexpr int kRgRun = AVEXHIP_REGIONS_RUN_FRAMES;               // frames per workgroup of the cells kernel
constexpr int kRgWords = AVEXHIP_REGIONS_WORDS;
constexpr int64_t kRgMax = 0x7fffffffll;
constexpr int kRgNone = 0x7fffffff;

// grid: one workgroup per run (avexhip_regions_recording::first_run numbers them), 256 threads.  LDS: 8 224 + 18 432 + 4 096 bytes.
__global__ __launch_bounds__(256) void regions_cells_kernel(const float* __restrict__ wav, const avexhip_regions_recording* __restrict__ rec, int n_rec, int hop,
                                                            int lo, int hi, const float* __restrict__ thr, const float* __restrict__ tables,
                                                            int32_t* __restrict__ cells, int32_t* __restrict__ nonfinite) {
    const FramePowerLds lds = frame_power_lds();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = last_at_most(n_rec, (int)blockIdx.x, [&](int i) { return rec[i].first_run; });
    const avexhip_regions_recording it = rec[r];
    const int64_t F = frames_of(it.n_samples, hop);
    const int64_t f0 = (int64_t)((int)blockIdx.x - it.first_run) * kRgRun;      // the run's first frame, counted inside its recording
    if (f0 >= F) return;                                         // (block-uniform; the entry point launches no such workgroup)
    const int nf = F - f0 < kRgRun ? (int)(F - f0) : kRgRun;

    stage_twiddles(lds.tw, tables);

    // lane l owns the bins l + 64 q; lane 0 bin 256 as well
    float t[5];
    bool in_band[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int k = lane + 64 * q;
        in_band[q] = k < kRecBins && k >= lo && k < hi;
        t[q] = k < kRecBins ? thr[(int64_t)r * kRecBins + k] : 0.f;
    }
    int n_bad = 0;                                               // (lane 0 of each wave counts its frames)

    const int64_t r_lo = it.base, r_hi = it.base + it.n_samples;
    for (int st = 0; st < nf; st += kFpStep) {                   // (block-uniform trip count)
        const int ns = nf - st < kFpStep ? nf - st : kFpStep;
        __syncthreads();                                         // the step before has read span
        // ---- the span of the step's frames -> LDS: lead <= 3, (ns - 1) hop + 512 <= 3 * 512 + 512 ---------------------------------------
        const int lead = stage_span(lds.span, wav, it.base + (f0 + st) * hop, (ns - 1) * hop + kRecFrame, r_lo, r_hi);
        __syncthreads();

        if (wave < ns) {                                         // (wave-uniform; only wave syncs and ballots inside)
            float p[5] = {0.f, 0.f, 0.f, 0.f, 0.f};              // (in_band is false where the lane has no bin)
            const bool bad = wave_frame_power(lds.span + lead + wave * hop, tables, lds.zbuf[wave], lds.tw, lane, [&](int q, int, float pk) { p[q] = pk; });
            unsigned mine = 0u;                                  // lane w < 9: word w of the frame
#pragma unroll
            for (int q = 0; q < 5; ++q) {                        // (every lane takes part in the ballots: lanes 1 .. 63 have no fifth bin)
                const unsigned long long m = __ballot(in_band[q] && p[q] > t[q]);      // false for a NaN on either side
                if (lane == 2 * q) mine = (unsigned)m;
                if (lane == 2 * q + 1) mine = (unsigned)(m >> 32);
            }
            if (lane < kRgWords) cells[(it.first_frame + f0 + st + wave) * kRgWords + lane] = (int32_t)mine;
            n_bad += bad ? 1 : 0;
        }
    }
    if (lane == 0 && n_bad) atomicAdd(nonfinite + r, n_bad);
}

// grid: one wave per frame, four frames per workgroup
__global__ __launch_bounds__(256) void regions_pack_kernel(const uint8_t* __restrict__ mask, int64_t total_frames, int32_t* __restrict__ cells) {
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= total_frames) return;                               // (wave-uniform)
    unsigned mine = 0u;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int k = lane + 64 * q;
        const bool set = k < kRecBins && mask[f * kRecBins + k] != 0;
        const unsigned long long m = __ballot(set);
        if (lane == 2 * q) mine = (unsigned)m;
        if (lane == 2 * q + 1) mine = (unsigned)(m >> 32);
    }
    if (lane < kRgWords) cells[f * kRgWords + lane] = (int32_t)mine;
}

// ---- what the prefix counts (prefix_count.h) -----------------------------------------------------------------------------------------------
struct RgFrameCells {            // the set cells of frame i
    const int32_t* cells;
    __device__ __forceinline__ int operator()(int64_t i) const {
        int c = 0;
#pragma unroll
        for (int w = 0; w < kRgWords; ++w) c += __popc((unsigned)cells[i * kRgWords + w]);
        return c;
    }
};
struct RgIsRoot {
    const int32_t* parent;
    __device__ __forceinline__ int operator()(int64_t i) const { return parent[i] == i ? 1 : 0; }
};
struct RgKept {                  // region i passes the filters
    const int32_t *cnt, *firstf, *lastf, *lowb, *highb;
    avexhip_regions_rule rule;
    __device__ __forceinline__ int operator()(int64_t i) const {
        const int nf = lastf[i] - firstf[i] + 1, nb = highb[i] - lowb[i] + 1;
        return cnt[i] >= rule.min_cells && nf >= rule.min_frames && nb >= rule.min_bins && (rule.max_frames < 0 || nf <= rule.max_frames) ? 1 : 0;
    }
};

// ---- union-find over the compact cells ---------------------------------------------------------------------------------------------------
struct CellWs {
    int32_t *parent, *rank, *cnt, *firstf, *lastf, *lowb, *highb, *recof, *pos;      // [n] each; from cnt on by region
    int32_t* block;              // [ceil(n / 1024)]
    size_t bytes;
};
struct FrameWs {
    int32_t* offset;             // [F] the set cells of the frames in front
    int32_t* block;              // [ceil(F / 1024)]
    size_t bytes;
};

static CellWs carve_cells(void* ws, int64_t n) {
    CellWs w;
    char* p = (char*)ws;
    int32_t** const arrays[9] = {&w.parent, &w.rank, &w.cnt, &w.firstf, &w.lastf, &w.lowb, &w.highb, &w.recof, &w.pos};
    for (int32_t** a : arrays) *a = take<int32_t>(p, (size_t)n);
    w.block = take<int32_t>(p, (size_t)prefix_count_blocks(n));
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

static FrameWs carve_frames(void* ws, int64_t F) {
    FrameWs w;
    char* p = (char*)ws;
    w.offset = take<int32_t>(p, (size_t)F);
    w.block = take<int32_t>(p, (size_t)prefix_count_blocks(F));
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

__global__ __launch_bounds__(256) void regions_init_kernel(int64_t n, CellWs w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    w.parent[i] = (int32_t)i;
    w.cnt[i] = 0;
    w.lastf[i] = 0;
    w.lowb[i] = kRgNone;
    w.highb[i] = 0;
}

// the root of x; on the way every cell of the path is pointed at its grandparent (path splitting, by atomicMin: a word only decreases)
__device__ __forceinline__ int rg_find(int32_t* parent, int x) {
    int p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);
    while (p < x) {
        const int gp = __atomic_load_n(parent + p, __ATOMIC_RELAXED);
        if (gp < p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void rg_unite(int32_t* parent, int a, int b) {
    for (;;) {
        a = rg_find(parent, a);
        b = rg_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = atomicMin(parent + a, b);                // a > b
        if (old == a) return;                                    // a was a root and hangs under b now
        a = old;                                                 // a had been hooked meanwhile: its other parent and b are still to be joined
    }
}

// lane w < 9: word w of frame g and the compact number of the frame's first cell at or above bin 32 w -> LDS.  Every lane of the wave
// makes the call.
__device__ __forceinline__ void rg_stage_frame(const int32_t* __restrict__ cells, const int32_t* __restrict__ offset, int64_t g, int lane, unsigned* words,
                                               int* first) {
    const unsigned w = lane < kRgWords ? (unsigned)cells[g * kRgWords + lane] : 0u;
    const int c = __popc(w);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane < kRgWords) {
        words[lane] = w;
        first[lane] = offset[g] + incl - c;
    }
}
__device__ __forceinline__ bool rg_bit(const unsigned* words, int k) { return (words[k >> 5] >> (k & 31)) & 1u; }
__device__ __forceinline__ int rg_number(const unsigned* words, const int* first, int k) {
    return first[k >> 5] + __popc(words[k >> 5] & ((1u << (k & 31)) - 1u));
}

// grid: one wave per frame, four frames per workgroup; every wave passes every barrier.
__global__ __launch_bounds__(256) void regions_union_kernel(const int32_t* __restrict__ cells, const int32_t* __restrict__ offset,
                                                            const int64_t* __restrict__ frame_offsets, int n_rec, int64_t total_frames, int rt, int rk,
                                                            int32_t* parent) {
    __shared__ unsigned own_w[4][kRgWords], nb_w[4][kRgWords];
    __shared__ int own_f[4][kRgWords], nb_f[4][kRgWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 4 + wave;
    const bool valid = f < total_frames;                         // (wave-uniform)
    int64_t f_end = 0;                                           // the end of the frame's recording
    if (valid) {
        const int r = last_at_most(n_rec, (int)f, [&](int i) { return frame_offsets[i]; });
        f_end = frame_offsets[r + 1];
        rg_stage_frame(cells, offset, f, lane, own_w[wave], own_f[wave]);
    }
    __syncthreads();
    for (int df = 0; df <= rt; ++df) {                           // (block-uniform trip count)
        const int64_t g = f + df;
        const bool has = valid && g < f_end;                     // (wave-uniform)
        if (df > 0) {
            __syncthreads();                                     // the step before has read nb
            if (has) rg_stage_frame(cells, offset, g, lane, nb_w[wave], nb_f[wave]);
            __syncthreads();
        }
        if (!has) continue;
        const unsigned* ow = own_w[wave];
        const int* of = own_f[wave];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int k = lane + 64 * q;
            if (k >= kRecBins || !rg_bit(ow, k)) continue;
            const int i = rg_number(ow, of, k);
            if (df == 0) {
                for (int dk = 1; dk <= rk; ++dk) {
                    const int k2 = k + dk;
                    if (k2 < kRecBins && rg_bit(ow, k2)) {       // the nearest one: the others hang on it
                        rg_unite(parent, i, rg_number(ow, of, k2));
                        break;
                    }
                }
            } else {
                const unsigned* nw = nb_w[wave];
                const int* nfirst = nb_f[wave];
                for (int dk = -rk; dk <= rk; ++dk) {
                    const int k2 = k + dk;
                    if (k2 < 0 || k2 >= kRecBins || !rg_bit(nw, k2)) continue;
                    if (dk > -rk && k2 > 0 && rg_bit(nw, k2 - 1)) continue;      // inside a run of set bits (rk >= 1 here): its first cell carries it
                    rg_unite(parent, i, rg_number(nw, nfirst, k2));
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void regions_flatten_kernel(int64_t n, int32_t* parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = rg_find(parent, (int)i);
    if (r != (int)i) __atomic_store_n(parent + i, r, __ATOMIC_RELAXED);
}

// grid: one wave per frame, four frames per workgroup.  rank[root] = the region's number.
__global__ __launch_bounds__(256) void regions_boxes_kernel(const int32_t* __restrict__ cells, const int32_t* __restrict__ offset,
                                                            const int64_t* __restrict__ frame_offsets, int n_rec, int64_t total_frames, CellWs w) {
    __shared__ unsigned own_w[4][kRgWords];
    __shared__ int own_f[4][kRgWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 4 + wave;
    const bool valid = f < total_frames;                         // (wave-uniform)
    if (valid) rg_stage_frame(cells, offset, f, lane, own_w[wave], own_f[wave]);
    __syncthreads();
    if (!valid) return;
    const int r = last_at_most(n_rec, (int)f, [&](int i) { return frame_offsets[i]; });
    const int fl = (int)(f - frame_offsets[r]);                  // on the recording's grid
    const unsigned* ow = own_w[wave];
    const int* of = own_f[wave];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int k = lane + 64 * q;
        const bool set = k < kRecBins && rg_bit(ow, k);
        int g = -1;
        if (set) {
            const int i = rg_number(ow, of, k), root = w.parent[i];
            g = w.rank[root];
            if (root == i) {                                     // the region's smallest cell
                w.firstf[g] = fl;
                w.recof[g] = r;
            }
        }
        unsigned long long todo = __ballot(set);
        while (todo) {                                           // (wave-uniform)
            const int leader = __ffsll((long long)todo) - 1;
            const int lg = __shfl(g, leader);
            const bool same = set && g == lg;
            const unsigned long long m = __ballot(same);
            const int k_lo = wave_reduce(same ? k : kRgNone, BlockMin()), k_hi = wave_reduce(same ? k : -1, BlockMax());
            if (lane == leader) {
                atomicAdd(w.cnt + lg, (int)__popcll(m));
                atomicMin(w.lowb + lg, k_lo);
                atomicMax(w.highb + lg, k_hi);
                atomicMax(w.lastf + lg, fl);
            }
            todo &= ~m;
        }
    }
}

// rows: [8, n_kept] in the order of AVEXHIP_REGIONS_COLUMNS
__global__ __launch_bounds__(256) void regions_rows_kernel(int64_t n_host, const int64_t* __restrict__ n_dev, RgKept kept, const int32_t* __restrict__ recof,
                                                           const int32_t* __restrict__ pos, int64_t n_kept, int32_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= prefix_n(n_host, n_dev) || !kept(i)) return;
    const int64_t o = pos[i];
    if (o < 0 || o >= n_kept) return;
    const int first = kept.firstf[i], last = kept.lastf[i], low = kept.lowb[i], high = kept.highb[i];
    const int v[AVEXHIP_REGIONS_COLUMNS] = {recof[i], first, last, low, high, kept.cnt[i], last - first + 1, high - low + 1};
#pragma unroll
    for (int c = 0; c < AVEXHIP_REGIONS_COLUMNS; ++c) rows[c * n_kept + o] = v[c];
}

// ---- what the entry points refuse ----------------------------------------------------------------------------------------------------------
int rg_recordings_check(const char* what, const avexhip_regions_recording* rec_host, const avexhip_regions_recording* rec_dev, int n_rec, int hop,
                        int64_t wav_samples, int64_t total_frames, int64_t* runs_out) {
    AVXH_TRY(table_check(what, rec_host, rec_dev, "rec_dev", n_rec, true, hop));
    int64_t frames = 0, runs = 0;
    for (int r = 0; r < n_rec; ++r) {
        const avexhip_regions_recording& it = rec_host[r];
        AVXH_TRY(recording_check(what, r, it.n_samples, it.base, wav_samples));
        AVX_REQUIRE(it.first_frame == frames && (int64_t)it.first_run == runs, "%s: recording %d: first_frame=%lld first_run=%d, expected %lld and %lld", what, r,
                    (long long)it.first_frame, it.first_run, (long long)frames, (long long)runs);
        const int64_t F = frames_of(it.n_samples, hop);
        frames += F;
        runs += (F + kRgRun - 1) / kRgRun;
        AVX_REQUIRE(frames <= kRgMax, "%s: more than 2^31 - 1 frames", what);
    }
    AVX_REQUIRE(total_frames == frames, "%s: total_frames=%lld, the table holds %lld", what, (long long)total_frames, (long long)frames);
    *runs_out = runs;
    return AVEXHIP_OK;
}

int rg_rule_check(const char* what, const avexhip_regions_rule* rule) {
    AVX_REQUIRE(rule, "%s: null argument", what);
    AVX_REQUIRE(rule->rt >= 0 && rule->rt <= AVEXHIP_REGIONS_MAX_RT && rule->rk >= 0 && rule->rk <= AVEXHIP_REGIONS_MAX_RK,
                "%s: reach (%d, %d) outside 0..%d frames and 0..%d bins", what, rule->rt, rule->rk, AVEXHIP_REGIONS_MAX_RT, AVEXHIP_REGIONS_MAX_RK);
    AVX_REQUIRE(rule->min_cells >= 1 && rule->min_frames >= 1 && rule->min_bins >= 1 && (rule->max_frames == -1 || rule->max_frames >= 1),
                "%s: min_cells=%d min_frames=%d min_bins=%d max_frames=%d: each >= 1 expected (max_frames -1: none)", what, rule->min_cells, rule->min_frames,
                rule->min_bins, rule->max_frames);
    return AVEXHIP_OK;
}

int rg_cells_count_check(const char* what, int64_t n_cells, int64_t total_frames) {
    AVX_REQUIRE(n_cells <= kRgMax, "%s: %lld set cells: more than 2^31 - 1; raise the threshold (snr_db, min_db) or take fewer recordings per call", what,
                (long long)n_cells);
    AVX_REQUIRE(n_cells >= 0 && (total_frames < 0 || n_cells <= total_frames * kRecBins), "%s: n_cells=%lld for %lld frames", what, (long long)n_cells,
                (long long)total_frames);
    return AVEXHIP_OK;
}

int rg_workspace_check(const char* what, const char* name, const void* ws, size_t have, size_t need) {
    AVX_REQUIRE(ws && aligned(ws, 8), "%s: %s must be 8-byte aligned and not null", what, name);
    if (have < need) {
        avexhip_set_error("%s: %s %zu B < %zu B", what, name, have, need);
        return AVEXHIP_ERR_WORKSPACE;
    }
    return AVEXHIP_OK;
}

unsigned rg_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" size_t avexhip_regions_workspace_bytes(int64_t total_frames, int64_t n_cells) {
    if (total_frames < 0 || total_frames > kRgMax || n_cells < 0 || n_cells > kRgMax) return 0;
    return (total_frames ? carve_frames(nullptr, total_frames).bytes : 0) + (n_cells ? carve_cells(nullptr, n_cells).bytes : 0);
}

extern "C" int avexhip_regions_cells(const float* wav_dev, int64_t wav_samples, const avexhip_regions_recording* rec_host,
                                     const avexhip_regions_recording* rec_dev, int n_rec, int hop, int lo, int hi, const float* thr_dev,
                                     const float* tables_dev, int64_t total_frames, int32_t* cells_dev, int32_t* nonfinite_dev, void* stream) {
    AVX_REQUIRE(wav_dev && tables_dev && thr_dev && nonfinite_dev, "regions_cells: null argument");
    AVX_REQUIRE(aligned(wav_dev, 16) && aligned(tables_dev, 16) && aligned(thr_dev, 4) && aligned(cells_dev, 4) && aligned(nonfinite_dev, 4),
                "regions_cells: wav_dev and tables_dev must be 16-byte aligned, thr_dev, cells_dev and nonfinite_dev 4-byte aligned");
    AVX_REQUIRE(wav_samples >= 1, "regions_cells: wav_samples=%lld", (long long)wav_samples);
    AVXH_TRY(bin_band_check("regions_cells", "band", -1, lo, hi));
    int64_t runs = 0;
    AVXH_TRY(rg_recordings_check("regions_cells", rec_host, rec_dev, n_rec, hop, wav_samples, total_frames, &runs));
    hipStream_t s = (hipStream_t)stream;
    AVX_HIP_CHECK(hipMemsetAsync(nonfinite_dev, 0, (size_t)n_rec * 4, s));
    if (runs == 0) return AVEXHIP_OK;                            // no recording holds a frame
    AVX_REQUIRE(cells_dev, "regions_cells: null argument");
    hipLaunchKernelGGL(regions_cells_kernel, dim3((unsigned)runs), dim3(256), 0, s, wav_dev, rec_dev, n_rec, hop, lo, hi, thr_dev, tables_dev, cells_dev,
                       nonfinite_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_regions_pack(const uint8_t* mask_dev, int64_t total_frames, int32_t* cells_dev, void* stream) {
    AVX_REQUIRE(total_frames >= 0 && total_frames <= kRgMax, "regions_pack: total_frames=%lld outside 0..2^31 - 1", (long long)total_frames);
    if (total_frames == 0) return AVEXHIP_OK;
    AVX_REQUIRE(mask_dev && cells_dev && aligned(cells_dev, 4), "regions_pack: null argument, or cells_dev not 4-byte aligned");
    regions_pack_kernel<<<dim3(rg_blocks(total_frames, 4)), dim3(256), 0, (hipStream_t)stream>>>(mask_dev, total_frames, cells_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_regions_count(const int32_t* cells_dev, int64_t total_frames, void* frame_ws_dev, size_t frame_ws_bytes, int64_t* counts_dev,
                                     void* stream) {
    AVX_REQUIRE(total_frames >= 0 && total_frames <= kRgMax, "regions_count: total_frames=%lld outside 0..2^31 - 1", (long long)total_frames);
    AVX_REQUIRE(counts_dev && aligned(counts_dev, 8), "regions_count: counts_dev must be 8-byte aligned and not null");
    hipStream_t s = (hipStream_t)stream;
    if (total_frames == 0) {
        AVX_HIP_CHECK(hipMemsetAsync(counts_dev, 0, 8, s));
        return AVEXHIP_OK;
    }
    AVX_REQUIRE(cells_dev && aligned(cells_dev, 4), "regions_count: cells_dev must be 4-byte aligned and not null");
    const FrameWs fw = carve_frames(frame_ws_dev, total_frames);
    AVXH_TRY(rg_workspace_check("regions_count", "frame workspace", frame_ws_dev, frame_ws_bytes, fw.bytes));
    return prefix_count<int64_t>(total_frames, PrefixDevN{total_frames, nullptr}, RgFrameCells{cells_dev}, fw.block, counts_dev, PrefixStoreRank{fw.offset}, s);
}

extern "C" int avexhip_regions_label(const int32_t* cells_dev, const int64_t* frame_offsets_host, const int64_t* frame_offsets_dev, int n_rec,
                                     int64_t total_frames, int64_t n_cells, const avexhip_regions_rule* rule, const void* frame_ws_dev,
                                     size_t frame_ws_bytes, void* cell_ws_dev, size_t cell_ws_bytes, int64_t* counts_dev, void* stream) {
    AVX_REQUIRE(frame_offsets_host && frame_offsets_dev && aligned(frame_offsets_dev, 8), "regions_label: frame_offsets must be 8-byte aligned and not null");
    AVX_REQUIRE(counts_dev && aligned(counts_dev, 8), "regions_label: counts_dev must be 8-byte aligned and not null");
    AVX_REQUIRE(n_rec >= 1, "regions_label: n_rec=%d", n_rec);
    AVXH_TRY(rg_rule_check("regions_label", rule));
    AVX_REQUIRE(frame_offsets_host[0] == 0, "regions_label: frame_offsets[0]=%lld, 0 expected", (long long)frame_offsets_host[0]);
    for (int r = 0; r < n_rec; ++r) {
        AVX_REQUIRE(frame_offsets_host[r + 1] >= frame_offsets_host[r], "regions_label: frame_offsets[%d]=%lld after %lld: the table is not in order", r + 1,
                    (long long)frame_offsets_host[r + 1], (long long)frame_offsets_host[r]);
        AVX_REQUIRE(frame_offsets_host[r + 1] <= kRgMax, "regions_label: more than 2^31 - 1 frames");
    }
    AVX_REQUIRE(frame_offsets_host[n_rec] == total_frames, "regions_label: total_frames=%lld, the table holds %lld", (long long)total_frames,
                (long long)frame_offsets_host[n_rec]);
    AVXH_TRY(rg_cells_count_check("regions_label", n_cells, total_frames));
    hipStream_t s = (hipStream_t)stream;
    if (n_cells == 0) {                                          // no region
        AVX_HIP_CHECK(hipMemsetAsync(counts_dev + 1, 0, 16, s));
        return AVEXHIP_OK;
    }
    AVX_REQUIRE(cells_dev && aligned(cells_dev, 4), "regions_label: cells_dev must be 4-byte aligned and not null");
    const FrameWs fw = carve_frames((void*)frame_ws_dev, total_frames);
    AVXH_TRY(rg_workspace_check("regions_label", "frame workspace", frame_ws_dev, frame_ws_bytes, fw.bytes));
    const CellWs cw = carve_cells(cell_ws_dev, n_cells);
    AVXH_TRY(rg_workspace_check("regions_label", "cell workspace", cell_ws_dev, cell_ws_bytes, cw.bytes));

    const dim3 per_cell(rg_blocks(n_cells, 256)), per_frame(rg_blocks(total_frames, 4));
    regions_init_kernel<<<per_cell, dim3(256), 0, s>>>(n_cells, cw);
    AVX_LAUNCH_CHECK();
    regions_union_kernel<<<per_frame, dim3(256), 0, s>>>(cells_dev, fw.offset, frame_offsets_dev, n_rec, total_frames, rule->rt, rule->rk, cw.parent);
    AVX_LAUNCH_CHECK();
    regions_flatten_kernel<<<per_cell, dim3(256), 0, s>>>(n_cells, cw.parent);
    AVX_LAUNCH_CHECK();
    AVXH_TRY(prefix_count<int64_t>(n_cells, PrefixDevN{n_cells, nullptr}, RgIsRoot{cw.parent}, cw.block, counts_dev + 1, PrefixStoreRank{cw.rank}, s));
    regions_boxes_kernel<<<per_frame, dim3(256), 0, s>>>(cells_dev, fw.offset, frame_offsets_dev, n_rec, total_frames, cw);
    AVX_LAUNCH_CHECK();
    return prefix_count<int64_t>(n_cells, PrefixDevN{n_cells, counts_dev + 1}, RgKept{cw.cnt, cw.firstf, cw.lastf, cw.lowb, cw.highb, *rule}, cw.block, counts_dev + 2,
                                 PrefixStoreRank{cw.pos}, s);
}

extern "C" int avexhip_regions_rows(int64_t n_cells, int64_t n_kept, const avexhip_regions_rule* rule, const void* cell_ws_dev, size_t cell_ws_bytes,
                                    const int64_t* counts_dev, int32_t* rows_dev, void* stream) {
    AVXH_TRY(rg_rule_check("regions_rows", rule));
    AVXH_TRY(rg_cells_count_check("regions_rows", n_cells, -1));
    AVX_REQUIRE(n_kept >= 0 && n_kept <= n_cells, "regions_rows: n_kept=%lld outside 0..%lld, the set cells", (long long)n_kept, (long long)n_cells);
    if (n_kept == 0) return AVEXHIP_OK;
    AVX_REQUIRE(counts_dev && aligned(counts_dev, 8) && rows_dev && aligned(rows_dev, 4),
                "regions_rows: counts_dev must be 8-byte aligned, rows_dev 4-byte aligned, neither null");
    const CellWs cw = carve_cells((void*)cell_ws_dev, n_cells);
    AVXH_TRY(rg_workspace_check("regions_rows", "cell workspace", cell_ws_dev, cell_ws_bytes, cw.bytes));
    regions_rows_kernel<<<dim3(rg_blocks(n_cells, 256)), dim3(256), 0, (hipStream_t)stream>>>(
        n_cells, counts_dev + 1, RgKept{cw.cnt, cw.firstf, cw.lastf, cw.lowb, cw.highb, *rule}, cw.recof, cw.pos, n_kept, rows_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
