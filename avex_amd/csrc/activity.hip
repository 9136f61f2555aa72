// Band-limited activity gate (ABI 21): "is there energy in this band above the recording's own noise floor", per sliding window, from
// the resident waveform of windows.hip -- the step the reference names and leaves empty (avex/preprocessing/activity_detector.py).
//   activity_frames_kernel   frames of 512 samples every `hop` -> periodic Hann, 512-point FFT, |X|^2 summed over each band's bins (fp32)
//   activity_floor_kernel    per (recording, band) the energy of a given rank among the recording's frames: an exact 8-bit radix select
//                            on the bit patterns (energies are >= +0, so the patterns order like the numbers; NaN sorts above +Inf)
//   activity_count_kernel    per (window, band) the frames with E > max(floor, floor_min) * ratio, and the largest energy
//   activity_select_kernel   window_select_kernel's condition and one more on those counts, through the same block_compact (block_prims.h)
// The transform is shared with fbank.hip (fft512.h): one wave64 per PAIR of frames packed as z = a + i b.  The walk over the frames is
// shared with soundscape.hip, measure.hip and regions.hip (rec_frames.h: the frame count, the workgroup's recording, the span and
// twiddle staging, the refusals of a table, a recording, a hop and a bin band): a workgroup takes eight consecutive frames of ONE
// recording and stages their span ((8 - 1) hop + 512 samples) in LDS once, so overlapping frames cost one HBM read per sample; pairs
// are (2 i, 2 i + 1) of the recording, so a frame's energies depend on its recording and the hop alone.
#include <math.h>

#include "block_prims.h"
#include "common.h"
#include "fft512.h"
#include "rec_frames.h"

namespace {

constexpr int kActBlockFrames = 8;               // frames per workgroup of the frames kernel: four waves, a pair each
constexpr int kActSpan = (kActBlockFrames - 1) * 512 + kRecFrame + 8;      // floats of LDS for the span at hop 512, up to 3 lead-in samples, a whole last chunk
constexpr int kFloorThreads = 1024;
constexpr int kActSelectThreads = 1024;

struct ActBands {
    int n;
    int lo[AVEXHIP_ACTIVITY_MAX_BANDS], hi[AVEXHIP_ACTIVITY_MAX_BANDS];      // bins lo .. hi - 1
};

// grid: one workgroup per eight frames of a recording (avexhip_activity_recording::first_block numbers them), 256 threads.
// tables: [512] window, then [512] (cos, -sin)(2 pi k / 512).
__global__ __launch_bounds__(256) void activity_frames_kernel(const float* __restrict__ wav, const avexhip_activity_recording* __restrict__ rec, int n_rec,
                                                              int hop, ActBands bands, const float* __restrict__ tables, int64_t total_frames,
                                                              float* __restrict__ energy) {
    __shared__ __attribute__((aligned(16))) float span[kActSpan];
    __shared__ float2 zbuf[4][8 * ZROW];
    __shared__ float2 tw[512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the recording of this workgroup: the last one whose first_block is <= blockIdx.x (recordings without a frame share their successor's)
    const avexhip_activity_recording it = rec[last_at_most(n_rec, (int)blockIdx.x, [&](int i) { return rec[i].first_block; })];
    const int64_t F = frames_of(it.n_samples, hop);
    const int64_t f0 = (int64_t)((int)blockIdx.x - it.first_block) * kActBlockFrames;
    if (f0 >= F) return;                                         // (block-uniform; the entry point launches no such workgroup)
    const int nf = F - f0 < kActBlockFrames ? (int)(F - f0) : kActBlockFrames;

    // ---- the span of the workgroup's frames -> LDS: lead <= 3, (nf - 1) hop + 512 <= 7 * 512 + 512 -----------------------------------------
    const int lead = stage_span(span, wav, it.base + f0 * hop, (nf - 1) * hop + kRecFrame, it.base, it.base + it.n_samples);
    stage_twiddles(tw, tables);
    __syncthreads();

    const int fa = 2 * wave;                                     // this wave's pair, counted inside the workgroup
    if (fa >= nf) return;                                        // (wave-uniform; no barrier follows)
    const bool has[2] = {true, fa + 1 < nf};
    float2* z = zbuf[wave];

    // ---- window; a frame that holds a NaN or an Inf is taken out of the transform (it would poison its partner) ----------------------
    float2 x[8];
    bool live[2], bad[2];
#pragma unroll
    for (int fr = 0; fr < 2; ++fr) {
        const float* src = span + lead + (has[fr] ? fa + fr : fa) * hop;
        float v[8];
        bool nonfin = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            v[q] = src[lane + 64 * q];
            nonfin |= non_finite(v[q]);
        }
        bad[fr] = has[fr] && __any(nonfin);
        const bool use = has[fr] && !bad[fr];
        bool nz = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float y = use ? v[q] * tables[lane + 64 * q] : 0.f;
            nz |= y != 0.f;
            if (fr == 0) x[q].x = y; else x[q].y = y;
        }
        // a frame that is exactly zero after the window comes out as +0 in every band: packed beside a loud partner its spectrum is the
        // difference of two large numbers and would pick up the partner's rounding noise (see fbank.hip)
        live[fr] = __any(nz);
    }

    fft512_wave(x, z, tw, lane);                                 // Z[k] at z[k]

    // ---- the two real spectra by conjugate symmetry (k = 0 and k = 256 pair with themselves), power, band sums -----------------------
    // A lane adds its bins of a band in increasing order, the wave its lanes by a butterfly: a fixed order, the same for every launch.
    float pa[5], pb[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int k = lane + 64 * q;
        pa[q] = 0.f; pb[q] = 0.f;
        if (k < kRecBins) {
            const float2 zk = z[k], zn = z[(512 - k) & 511];
            const float ar = 0.5f * (zk.x + zn.x), ai = 0.5f * (zk.y - zn.y);
            const float br = 0.5f * (zk.y + zn.y), bi = -0.5f * (zk.x - zn.x);
            pa[q] = ar * ar + ai * ai;
            pb[q] = br * br + bi * bi;
        }
    }
    const int64_t f_out = it.first_frame + f0 + fa;
    for (int b = 0; b < bands.n; ++b) {
        const int k_lo = bands.lo[b], k_hi = bands.hi[b];
        float ea = 0.f, eb = 0.f;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int k = lane + 64 * q;
            const bool in = k >= k_lo && k < k_hi;
            ea += in ? pa[q] : 0.f;
            eb += in ? pb[q] : 0.f;
        }
        ea = wave_sum(ea);
        eb = wave_sum(eb);
        if (lane == 0) {
            float* dst = energy + (int64_t)b * total_frames + f_out;
            dst[0] = bad[0] ? NAN : (live[0] ? ea : 0.f);
            if (has[1]) dst[1] = bad[1] ? NAN : (live[1] ? eb : 0.f);
        }
    }
}

// grid (n_rec, n_bands).  Four passes over the keys of the recording's frames, most significant byte first: a histogram of the byte among
// the keys that share the bytes chosen so far (integer LDS atomics, which only count), the byte whose bin holds the wanted rank.  After
// the fourth pass the prefix IS the key of that rank, whatever order the atomics ran in.
__global__ __launch_bounds__(kFloorThreads) void activity_floor_kernel(const float* __restrict__ energy, const avexhip_activity_recording* __restrict__ rec,
                                                                       int hop, int64_t total_frames, int n_bands, float* __restrict__ floor_out,
                                                                       int* __restrict__ nonfinite) {
    __shared__ int hist[256];
    __shared__ int sel_digit, sel_below, bad_total;
    const int tid = threadIdx.x, r = blockIdx.x, b = blockIdx.y;
    const avexhip_activity_recording it = rec[r];
    const int F = (int)frames_of(it.n_samples, hop);         // < 2^31 (checked on the host)
    if (F == 0) {                                                // (block-uniform)
        if (tid == 0) {
            floor_out[(int64_t)r * n_bands + b] = NAN;
            if (b == 0) nonfinite[r] = 0;
        }
        return;
    }
    const uint32_t* keys = (const uint32_t*)(energy + (int64_t)b * total_frames + it.first_frame);
    if (tid == 0) bad_total = 0;
    uint32_t prefix = 0u;
    int need = it.floor_rank;                                    // keys in front of the wanted one, among those that share the prefix
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        int n_bad = 0;
        for (int base = 0; base < F; base += 4 * kFloorThreads) {      // (block-uniform trip count: the ballots see whole waves)
            uint32_t key[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {                        // four loads in flight per thread
                const int i = base + q * kFloorThreads + tid;
                key[q] = i < F ? keys[i] : 0u;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = base + q * kFloorThreads + tid < F && (pass == 0 || (uint32_t)((uint64_t)key[q] >> (shift + 8)) == prefix);
                if (pass == 0 && in) n_bad += (key[q] & 0x7fffffffu) > 0x7f800000u ? 1 : 0;
                // The energies of a recording share their leading byte (one exponent range), and 64 atomics on one LDS word run one after the
                // other: the lanes that hold the first lane's byte are counted by a ballot and added once, the others add for themselves.
                const int dg = (int)((key[q] >> shift) & 255u);
                const unsigned long long counted = __ballot(in);
                if (counted == 0ull) continue;                   // (wave-uniform)
                const int leader = __ffsll((long long)counted) - 1;
                const int d0 = __shfl(dg, leader, 64);
                const unsigned long long same = __ballot(in && dg == d0);
                if ((tid & 63) == leader) atomicAdd(&hist[d0], (int)__popcll(same));
                else if (in && dg != d0) atomicAdd(&hist[dg], 1);
            }
        }
        if (pass == 0 && n_bad) atomicAdd(&bad_total, n_bad);
        __syncthreads();
        if (tid < 256) {
            int below = 0;
            for (int d = 0; d < tid; ++d) below += hist[d];
            if (below <= need && need < below + hist[tid]) {
                sel_digit = tid;
                sel_below = below;
            }
        }
        __syncthreads();
        need -= sel_below;
        prefix = (prefix << 8) | (uint32_t)sel_digit;
        __syncthreads();                                         // hist and sel_* are read; the next pass resets them
    }
    if (tid == 0) {
        floor_out[(int64_t)r * n_bands + b] = __uint_as_float(prefix);
        if (b == 0) nonfinite[r] = bad_total;
    }
}

// One wave per window: its frames are f_lo = ceil(start / hop) .. f_hi = floor((start + valid - 512) / hop) of its recording.
__global__ __launch_bounds__(64) void activity_count_kernel(const avexhip_window* __restrict__ win, const int* __restrict__ win_rec,
                                                            const avexhip_activity_recording* __restrict__ rec, int hop, const float* __restrict__ energy,
                                                            int64_t total_frames, const float* __restrict__ floor_in, int n_bands, float floor_min, float ratio,
                                                            int* __restrict__ n_frames, int* __restrict__ active, float* __restrict__ max_energy) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const avexhip_window it = win[w];
    const int r = win_rec[w];
    const int64_t first = rec[r].first_frame;
    const int64_t f_lo = (it.start + hop - 1) / hop;
    const int64_t end = it.start + it.valid - kRecFrame;
    const int64_t f_hi = end < 0 ? -1 : end / hop;
    const int nf = f_hi >= f_lo ? (int)(f_hi - f_lo + 1) : 0;
    if (lane == 0) n_frames[w] = nf;
    for (int b = 0; b < n_bands; ++b) {
        const float fl = floor_in[(int64_t)r * n_bands + b];
        const float thr = nan_max(floor_min, fl) * ratio;        // one fp32 multiply; a NaN floor stays NaN, and no compare with it holds
        const float* e = energy + (int64_t)b * total_frames + first + f_lo;
        int cnt = 0;
        float mx = -INFINITY;
        for (int i = lane; i < nf; i += 64) {
            const float v = e[i];
            cnt += v > thr ? 1 : 0;
            mx = nan_max(mx, v);
        }
        cnt = wave_reduce(cnt, BlockSum());
        mx = wave_reduce(mx, [](float a, float b) { return nan_max(a, b); });
        if (lane == 0) {
            active[(int64_t)w * n_bands + b] = cnt;
            max_energy[(int64_t)w * n_bands + b] = mx;
        }
    }
}

// window_select_kernel's predicate (windows.hip) with one more condition: active_frames >= min_active in any band (mode 0) or in every band (mode 1).
__global__ __launch_bounds__(kActSelectThreads) void activity_select_kernel(const avexhip_window* __restrict__ win, const double* __restrict__ energy,
                                                                            const float* __restrict__ peak, const int* __restrict__ active, int n_win,
                                                                            int n_bands, int min_active, int mode, double thr_energy, float thr_peak,
                                                                            int* __restrict__ kept, int* __restrict__ count) {
    block_compact<kActSelectThreads>(n_win, [&](int i) {
        const int valid = win[i].valid;
        const bool keep = valid > 0 && energy[i] >= thr_energy * (double)valid && peak[i] >= thr_peak;      // a NaN fails both compares
        int bands_ok = 0;
        for (int b = 0; b < n_bands; ++b) bands_ok += active[(int64_t)i * n_bands + b] >= min_active ? 1 : 0;
        return keep && (mode == 0 ? bands_ok > 0 : bands_ok == n_bands);
    }, kept, count);
}

// What every entry point refuses in the recording table; *blocks_out = the workgroups of the frames kernel.  wav_samples < 0: no buffer to check.
int activity_recordings_check(const char* what, const avexhip_activity_recording* rec_host, const avexhip_activity_recording* rec_dev, int n_rec, int hop,
                              int64_t wav_samples, int64_t total_frames, int64_t* blocks_out) {
    AVXH_TRY(table_check(what, rec_host, rec_dev, "rec_dev", n_rec, true, hop));
    int64_t frames = 0, blocks = 0;
    for (int r = 0; r < n_rec; ++r) {
        const avexhip_activity_recording& it = rec_host[r];
        AVXH_TRY(recording_check(what, r, it.n_samples, it.base, wav_samples));
        const int64_t F = frames_of(it.n_samples, hop);
        AVX_REQUIRE(it.first_frame == frames && (int64_t)it.first_block == blocks, "%s: recording %d: first_frame=%lld first_block=%d, expected %lld and %lld", what, r,
                    (long long)it.first_frame, it.first_block, (long long)frames, (long long)blocks);
        AVX_REQUIRE(it.floor_rank >= 0 && (int64_t)it.floor_rank < (F > 0 ? F : 1), "%s: recording %d: floor_rank=%d outside its %lld frames", what, r, it.floor_rank,
                    (long long)F);
        frames += F;
        blocks += (F + kActBlockFrames - 1) / kActBlockFrames;
        AVX_REQUIRE(frames < ((int64_t)1 << 31) && blocks < ((int64_t)1 << 31), "%s: more than 2^31 - 1 frames", what);
    }
    AVX_REQUIRE(total_frames == frames, "%s: total_frames=%lld, the table holds %lld", what, (long long)total_frames, (long long)frames);
    if (blocks_out) *blocks_out = blocks;
    return AVEXHIP_OK;
}

int activity_bands_check(const char* what, int n_bands) {
    AVX_REQUIRE(n_bands >= 1 && n_bands <= AVEXHIP_ACTIVITY_MAX_BANDS, "%s: n_bands=%d outside 1..%d", what, n_bands, AVEXHIP_ACTIVITY_MAX_BANDS);
    return AVEXHIP_OK;
}

}  // namespace

extern "C" int avexhip_activity_frames(const float* wav_dev, int64_t wav_samples, const avexhip_activity_recording* rec_host,
                                       const avexhip_activity_recording* rec_dev, int n_rec, int hop, const int32_t* bands_host, int n_bands,
                                       const float* tables_dev, int64_t total_frames, float* energy_dev, void* stream) {
    AVX_REQUIRE(wav_dev && bands_host && tables_dev, "activity_frames: null argument");
    AVX_REQUIRE(aligned(wav_dev, 16) && aligned(tables_dev, 16) && aligned(energy_dev, 4),
                "activity_frames: wav_dev and tables_dev must be 16-byte aligned, energy_dev 4-byte aligned");
    AVX_REQUIRE(wav_samples >= 1, "activity_frames: wav_samples=%lld", (long long)wav_samples);
    AVXH_TRY(activity_bands_check("activity_frames", n_bands));
    ActBands bands;
    memset(&bands, 0, sizeof(bands));
    bands.n = n_bands;
    for (int b = 0; b < n_bands; ++b) {
        bands.lo[b] = bands_host[2 * b];
        bands.hi[b] = bands_host[2 * b + 1];
        AVXH_TRY(bin_band_check("activity_frames", "band", b, bands.lo[b], bands.hi[b]));
    }
    int64_t blocks = 0;
    AVXH_TRY(activity_recordings_check("activity_frames", rec_host, rec_dev, n_rec, hop, wav_samples, total_frames, &blocks));
    if (blocks == 0) return AVEXHIP_OK;                          // no recording holds a frame
    AVX_REQUIRE(energy_dev, "activity_frames: null argument");
    hipLaunchKernelGGL(activity_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, wav_dev, rec_dev, n_rec, hop, bands, tables_dev,
                       total_frames, energy_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_activity_floor(const float* energy_dev, int64_t total_frames, const avexhip_activity_recording* rec_host,
                                      const avexhip_activity_recording* rec_dev, int n_rec, int hop, int n_bands, float* floor_dev, int32_t* nonfinite_dev,
                                      void* stream) {
    AVX_REQUIRE(floor_dev && nonfinite_dev, "activity_floor: null argument");
    AVX_REQUIRE(aligned(energy_dev, 4) && aligned(floor_dev, 4) && aligned(nonfinite_dev, 4),
                "activity_floor: energy_dev, floor_dev and nonfinite_dev must be 4-byte aligned");
    AVXH_TRY(activity_bands_check("activity_floor", n_bands));
    AVXH_TRY(activity_recordings_check("activity_floor", rec_host, rec_dev, n_rec, hop, -1, total_frames, nullptr));
    AVX_REQUIRE(energy_dev || total_frames == 0, "activity_floor: null argument");
    hipLaunchKernelGGL(activity_floor_kernel, dim3((unsigned)n_rec, (unsigned)n_bands), dim3(kFloorThreads), 0, (hipStream_t)stream, energy_dev, rec_dev, hop,
                       total_frames, n_bands, floor_dev, nonfinite_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_activity_count(const avexhip_window* win_host, const avexhip_window* win_dev, const int32_t* win_rec_host, const int32_t* win_rec_dev,
                                      int n_win, const avexhip_activity_recording* rec_host, const avexhip_activity_recording* rec_dev, int n_rec, int hop,
                                      const float* energy_dev, int64_t total_frames, const float* floor_dev, int n_bands, float floor_min, float ratio,
                                      int32_t* n_frames_dev, int32_t* active_dev, float* max_energy_dev, void* stream) {
    AVX_REQUIRE(win_host && win_dev && win_rec_host && win_rec_dev && floor_dev && n_frames_dev && active_dev && max_energy_dev, "activity_count: null argument");
    AVX_REQUIRE(aligned(win_dev, 8) && aligned(win_rec_dev, 4) && aligned(energy_dev, 4) && aligned(floor_dev, 4) && aligned(n_frames_dev, 4) &&
                    aligned(active_dev, 4) && aligned(max_energy_dev, 4),
                "activity_count: win_dev must be 8-byte aligned, the other device arrays 4-byte aligned");
    AVX_REQUIRE(n_win >= 1, "activity_count: n_win=%d", n_win);
    AVX_REQUIRE(!(floor_min != floor_min) && !(ratio != ratio) && floor_min >= 0.f && ratio >= 0.f, "activity_count: floor_min=%g ratio=%g: numbers >= 0 expected (not NaN)",
                (double)floor_min, (double)ratio);
    AVXH_TRY(activity_bands_check("activity_count", n_bands));
    AVXH_TRY(activity_recordings_check("activity_count", rec_host, rec_dev, n_rec, hop, -1, total_frames, nullptr));
    AVX_REQUIRE(energy_dev || total_frames == 0, "activity_count: null argument");
    for (int w = 0; w < n_win; ++w) {
        const avexhip_window& it = win_host[w];
        const int r = win_rec_host[w];
        AVX_REQUIRE(r >= 0 && r < n_rec, "activity_count: window %d: recording %d outside the table's %d", w, r, n_rec);
        AVX_REQUIRE(it.base == rec_host[r].base && it.n_samples == rec_host[r].n_samples, "activity_count: window %d is not a window of recording %d", w, r);
        AVX_REQUIRE(it.valid >= 0 && it.start >= 0 && it.start <= it.n_samples - it.valid, "activity_count: window %d: %lld + %d leaves the recording's %lld samples", w,
                    (long long)it.start, it.valid, (long long)it.n_samples);
    }
    hipLaunchKernelGGL(activity_count_kernel, dim3((unsigned)n_win), dim3(64), 0, (hipStream_t)stream, win_dev, win_rec_dev, rec_dev, hop, energy_dev, total_frames,
                       floor_dev, n_bands, floor_min, ratio, n_frames_dev, active_dev, max_energy_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_activity_select(const avexhip_window* win_dev, const double* energy_dev, const float* peak_dev, const int32_t* active_dev, int n_win,
                                       int n_bands, int min_active_frames, int mode, double thr_energy, float thr_peak, int32_t* kept_dev, int32_t* count_dev,
                                       void* stream) {
    AVX_REQUIRE(win_dev && energy_dev && peak_dev && active_dev && kept_dev && count_dev, "activity_select: null argument");
    AVX_REQUIRE(aligned(win_dev, 8) && aligned(energy_dev, 8) && aligned(peak_dev, 4) && aligned(active_dev, 4) && aligned(kept_dev, 4) &&
                    aligned(count_dev, 4),
                "activity_select: win_dev and energy_dev must be 8-byte aligned, the other device arrays 4-byte aligned");
    AVX_REQUIRE(n_win >= 1, "activity_select: n_win=%d", n_win);
    AVXH_TRY(activity_bands_check("activity_select", n_bands));
    AVX_REQUIRE(min_active_frames >= 0, "activity_select: min_active_frames=%d", min_active_frames);
    AVX_REQUIRE(mode == AVEXHIP_ACTIVITY_ANY || mode == AVEXHIP_ACTIVITY_ALL, "activity_select: unknown mode %d", mode);
    AVX_REQUIRE(!(thr_energy != thr_energy) && !(thr_peak != thr_peak), "activity_select: a threshold is NaN (-inf turns one off)");
    hipLaunchKernelGGL(activity_select_kernel, dim3(1), dim3(kActSelectThreads), 0, (hipStream_t)stream, win_dev, energy_dev, peak_dev, active_dev, n_win, n_bands,
                       min_active_frames, mode, thr_energy, thr_peak, kept_dev, count_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
