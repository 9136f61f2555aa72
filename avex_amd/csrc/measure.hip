// Event measurements (ABI 24): the time and frequency extent of each event, from the resident waveform of windows.hip and the frames of
// soundscape.hip (512 samples every `hop`, periodic Hann, no padding, ONE frame per transform: P[f, k] comes from wave_frame_power of
// frame_power.h, the text soundscape_stats_kernel runs, so it is the same bits).  An event is a box: the samples [s0, s1) of one recording and the
// bins [lo, hi); its frames are those that lie wholly inside [s0, s1).
//   measure_frames_kernel   a run of up to 64 consecutive frames of ONE event per workgroup: |X|^2 per frame and bin, per bin the sum
//                           over the run in frame order (one partial row per run, with the run's non-finite frames), and per frame
//                           the band energy -> envelope (a lane adds its bins in increasing order, then the wave butterfly: with the
//                           full band the bits of soundscape's frame_power)
//   measure_reduce_kernel   one workgroup per event: the runs' partials in run order -> spectrum, then fp64: the noise subtraction,
//                           the cumulative sum over the bins (block_scan) -> the quantile bins and the peak; two passes over the
//                           envelope in chunks of 256 frames with a carry (the total, then the quantile frames) and its peak
// No atomics, sums in one fixed order: an event's numbers depend on its recording's samples, its box, hop, the quantile levels and
// its noise row alone -- the same bits in any company, in any order of the events and on every run.  The walk over the frames is
// rec_frames.h's (the frame count, the event of a run, the span and twiddle staging, the refusals of a table, a recording, a hop, a bin
// band and a short buffer of partials); every partial row, envelope value and frame index follows from the checked table.
#include <math.h>

#include "block_prims.h"
#include "common.h"
#include "frame_power.h"

namespace {

constexpr int kMsRun = AVEXHIP_MEASURE_RUN_FRAMES;               // frames per workgroup of the frames kernel
// a partial row, in 4-byte words: the 257 sums, the run's non-finite frames
constexpr int kMsPartBad = kRecBins, kMsPartWords = kRecBins + 1;
constexpr int kMsNone = 0x7fffffff;                              // "no index": the identity of the minimum over indices

__host__ __device__ __forceinline__ int64_t ms_first_frame(int64_t s0, int hop) { return (s0 + hop - 1) / hop; }
// the frames of the box [s0, s1) of a recording of F frames: those that lie wholly inside
__host__ __device__ __forceinline__ int64_t ms_frames(int64_t s0, int64_t s1, int hop, int64_t F) {
    int64_t f1 = s1 >= kRecFrame ? (s1 - kRecFrame) / hop + 1 : 0;
    f1 = f1 < F ? f1 : F;
    const int64_t n = f1 - ms_first_frame(s0, hop);
    return n > 0 ? n : 0;
}

// grid: one workgroup per run (avexhip_measure_event::first_run numbers them), 256 threads.  tables: [512] window, then [512]
// (cos, -sin)(2 pi k / 512).  LDS: 8 224 + 18 432 + 4 096 + 4 160 + 16 bytes = 34 928.
__global__ __launch_bounds__(256) void measure_frames_kernel(const float* __restrict__ wav, const avexhip_measure_event* __restrict__ ev, int n_ev, int hop,
                                                             const float* __restrict__ tables, float* __restrict__ partials, float* __restrict__ envelope) {
    const FramePowerLds lds = frame_power_lds();
    __shared__ float prow[kFpStep][kFpPRow];
    __shared__ int bad_of[kFpStep];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = last_at_most(n_ev, (int)blockIdx.x, [&](int i) { return ev[i].first_run; });
    const avexhip_measure_event it = ev[e];
    const int in_ev = ((int)blockIdx.x - it.first_run) * kMsRun;   // the run's first frame, counted inside its event
    if (in_ev < 0 || in_ev >= it.n_frames) return;               // (block-uniform; the entry point launches no such workgroup)
    const int nf = it.n_frames - in_ev < kMsRun ? it.n_frames - in_ev : kMsRun;
    const int64_t f0 = ms_first_frame(it.s0, hop) + in_ev;       // the run's first frame, counted inside its recording
    const int lo = it.lo, hi = it.hi;

    stage_twiddles(lds.tw, tables);

    // thread t owns bin t; thread 0 bin 256 as well
    const int n_own = tid == 0 ? 2 : 1;
    float s_pow[2] = {0.f, 0.f};
    int n_bad = 0;

    const int64_t r_lo = it.base, r_hi = it.base + it.n_samples;
    for (int st = 0; st < nf; st += kFpStep) {                   // (block-uniform trip count)
        const int ns = nf - st < kFpStep ? nf - st : kFpStep;
        __syncthreads();                                         // the step before has read span and prow
        // ---- the span of the step's frames -> LDS: lead <= 3, (ns - 1) hop + 512 <= 3 * 512 + 512 ---------------------------------------
        const int lead = stage_span(lds.span, wav, it.base + (f0 + st) * hop, (ns - 1) * hop + kRecFrame, r_lo, r_hi);
        __syncthreads();

        if (wave < ns) {                                         // (wave-uniform; only wave syncs inside)
            // A lane adds its bins in increasing order, the wave its lanes by a butterfly: a fixed order, the same for every launch.
            // A bin outside the band adds +0, which changes no bit of the sum.
            float total = 0.f;
            const bool bad = wave_frame_power(lds.span + lead + wave * hop, tables, lds.zbuf[wave], lds.tw, lane, [&](int, int k, float p) {
                prow[wave][k] = p;
                total += (k >= lo && k < hi) ? p : 0.f;
            });
            total = wave_sum(total);
            if (lane == 0) {
                envelope[it.env_offset + in_ev + st + wave] = total;
                bad_of[wave] = bad ? 1 : 0;
            }
        }
        __syncthreads();

        // ---- the step's frames into the bin owners' sums, in frame order ------------------------------------------------------------------
        for (int j = 0; j < ns; ++j) {
#pragma unroll
            for (int o = 0; o < 2; ++o)
                if (o < n_own) s_pow[o] += prow[j][o == 0 ? tid : 256];
            if (tid == 0) n_bad += bad_of[j];
        }
    }

    float* part = partials + (int64_t)blockIdx.x * kMsPartWords;
    part[tid] = s_pow[0];
    if (tid == 0) {
        part[256] = s_pow[1];
        ((int*)part)[kMsPartBad] = n_bad;
    }
}

// d = a value minus its noise: what is left of it, never below 0; a NaN (from a NaN noise row) stays one
__device__ __forceinline__ double ms_left(double d) { return d <= 0.0 ? 0.0 : d; }

// grid: one workgroup per event, 256 threads; thread t owns bin t, thread 0 bin 256 as well.  noise: [n_rec, 257] or null.
__global__ __launch_bounds__(256) void measure_reduce_kernel(const avexhip_measure_event* __restrict__ ev, int hop, const float* __restrict__ partials,
                                                             const float* __restrict__ envelope, const float* __restrict__ noise, double q_lo, double q_c,
                                                             double q_hi, float* __restrict__ spectrum, avexhip_measure_result out) {
    __shared__ double wt[4], wmax[4], noise_band;
    __shared__ int wi[4][4], wbad[4];
    const int e = blockIdx.x, tid = threadIdx.x;
    const avexhip_measure_event it = ev[e];
    const int n = it.n_frames, lo = it.lo, hi = it.hi;
    const int n_runs = (n + kMsRun - 1) / kMsRun;
    const float* part0 = partials + (int64_t)it.first_run * kMsPartWords;
    const double qs[3] = {q_lo, q_c, q_hi};

    int v_bad = 0;
    for (int u = tid; u < n_runs; u += 256) v_bad += ((const int*)(part0 + (int64_t)u * kMsPartWords))[kMsPartBad];
    const int n_bad = block_reduce<4>(v_bad, BlockSum(), wbad);

    // ---- spectrum: the runs' partials in run order; +0 outside the band, NaN inside it with a non-finite frame ----------------------------
    const float* nz = noise ? noise + (int64_t)it.recording * kRecBins : nullptr;
    double sp[2] = {0.0, 0.0};                                   // S' of the thread's bins
    for (int o = 0; o < (tid == 0 ? 2 : 1); ++o) {
        const int k = o == 0 ? tid : 256;
        const bool in_band = k >= lo && k < hi;
        float s = 0.f;
        if (in_band)
            for (int u = 0; u < n_runs; ++u) s += part0[(int64_t)u * kMsPartWords + k];
        spectrum[(int64_t)e * kRecBins + k] = (in_band && n_bad) ? NAN : s;
        if (in_band) sp[o] = nz ? ms_left((double)s - (double)n * (double)nz[k]) : (double)s;
    }
    if (tid == 0) {
        double nb = 0.0;
        if (nz)
            for (int k = lo; k < hi; ++k) nb += (double)nz[k];   // in bin order
        noise_band = nb;
        out.n_frames[e] = n;
        out.nonfinite[e] = n_bad;
    }
    if (n == 0 || n_bad > 0) {                                   // (block-uniform) nothing to measure
        if (tid == 0) {
            out.energy[e] = NAN;
            out.snr_db[e] = NAN;
            out.low_bin[e] = out.centre_bin[e] = out.high_bin[e] = out.peak_bin[e] = -1;
            out.low_frame[e] = out.centre_frame[e] = out.high_frame[e] = out.peak_frame[e] = -1;
        }
        return;
    }

    // ---- the bins: cumulative sum in bin order, bin 256 behind the 256 threads' -------------------------------------------------------------
    double excl, total;
    const double incl = block_scan<4>(sp[0], 0.0, BlockSum(), wt, &excl, &total);
    __shared__ double s256;
    if (tid == 0) s256 = sp[1];
    const double own_max = block_reduce<4>(sp[0], BlockMax(), wmax);
    __syncthreads();                                             // s256 is written, wmax is read
    const double E = total + s256;
    const double top = s256 > own_max ? s256 : own_max;
    {
        // the smallest bin with C[k] >= q E for the three levels, and the lowest bin attaining the maximum
        int cand[4];
        const bool mine = tid >= lo && tid < hi;
#pragma unroll
        for (int j = 0; j < 3; ++j) cand[j] = (mine && incl >= qs[j] * E) ? tid : kMsNone;
        cand[3] = (mine && sp[0] == top) ? tid : kMsNone;
#pragma unroll
        for (int j = 0; j < 4; ++j) cand[j] = block_reduce<4>(cand[j], BlockMin(), wi[j]);
        if (tid == 0) {
            const bool any = E > 0.0;                            // false for a NaN
            const bool last = hi == kRecBins;                    // bin 256: C[256] = E
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (cand[j] == kMsNone && last && (j < 3 ? E >= qs[j] * E : s256 == top)) cand[j] = 256;
            out.energy[e] = E;
            out.low_bin[e] = any && cand[0] != kMsNone ? cand[0] : -1;
            out.centre_bin[e] = any && cand[1] != kMsNone ? cand[1] : -1;
            out.high_bin[e] = any && cand[2] != kMsNone ? cand[2] : -1;
            out.peak_bin[e] = any && cand[3] != kMsNone ? cand[3] : -1;
            const double den = (double)n * noise_band;
            out.snr_db[e] = (nz && den != 0.0) ? 10.0 * log10(E / den) : (double)NAN;
        }
    }
    __syncthreads();                                             // wt, wi: the passes below reuse them

    // ---- the frames: the total and the maximum, then the quantile frames, in chunks of 256 with a carry -----------------------------------
    const float* env = envelope + it.env_offset;
    const double nb = nz ? noise_band : 0.0;
    auto left_of = [&](int t) { return nz ? ms_left((double)env[t] - nb) : (double)env[t]; };
    double carry = 0.0, t_max = -1.0;
    for (int c = 0; c < n; c += 256) {                           // (block-uniform trip count)
        const int t = c + tid;
        const double v = t < n ? left_of(t) : 0.0;
        if (t < n && v > t_max) t_max = v;
        double ex, tot;
        block_scan<4>(v, 0.0, BlockSum(), wt, &ex, &tot);
        carry += tot;
    }
    const double T = carry;
    const double t_top = block_reduce<4>(t_max, BlockMax(), wmax);
    int cand[4] = {kMsNone, kMsNone, kMsNone, kMsNone};
    carry = 0.0;
    for (int c = 0; c < n; c += 256) {
        const int t = c + tid;
        const double v = t < n ? left_of(t) : 0.0;
        double ex, tot;
        const double inc = carry + block_scan<4>(v, 0.0, BlockSum(), wt, &ex, &tot);
        if (t < n) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (cand[j] == kMsNone && inc >= qs[j] * T) cand[j] = t;
            if (cand[3] == kMsNone && v == t_top) cand[3] = t;
        }
        carry += tot;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cand[j] = block_reduce<4>(cand[j], BlockMin(), wi[j]);
    if (tid == 0) {
        const bool any = T > 0.0;
        const int f0 = (int)ms_first_frame(it.s0, hop);          // < 2^31: the entry point checks the recording's frames
        out.low_frame[e] = any && cand[0] != kMsNone ? f0 + cand[0] : -1;
        out.centre_frame[e] = any && cand[1] != kMsNone ? f0 + cand[1] : -1;
        out.high_frame[e] = any && cand[2] != kMsNone ? f0 + cand[2] : -1;
        out.peak_frame[e] = any && cand[3] != kMsNone ? f0 + cand[3] : -1;
    }
}

// What both entry points refuse in the event table.  wav_samples < 0: no buffer to check; n_rec < 0: no noise rows to index.
int measure_events_check(const char* what, const avexhip_measure_event* ev_host, const avexhip_measure_event* ev_dev, int n_ev, int hop, int64_t wav_samples,
                         int n_rec, int64_t total_frames, int64_t total_runs) {
    AVXH_TRY(table_check(what, ev_host, ev_dev, "ev_dev", n_ev, false, hop));      // (the entry points return before this for n_ev == 0)
    int64_t frames = 0, runs = 0;
    for (int e = 0; e < n_ev; ++e) {
        const avexhip_measure_event& it = ev_host[e];
        AVXH_TRY(recording_check(what, e, it.n_samples, it.base, wav_samples));
        AVX_REQUIRE(it.s0 >= 0 && it.s0 <= it.s1 && it.s1 <= it.n_samples, "%s: event %d: samples %lld..%lld outside a recording of %lld", what, e,
                    (long long)it.s0, (long long)it.s1, (long long)it.n_samples);
        AVXH_TRY(bin_band_check(what, "event", e, it.lo, it.hi));
        AVX_REQUIRE(it.recording >= 0 && (n_rec < 0 || it.recording < n_rec), "%s: event %d: recording=%d outside 0..%d", what, e, it.recording, n_rec - 1);
        AVX_REQUIRE(frames_of(it.n_samples, hop) < ((int64_t)1 << 31), "%s: event %d: a recording of more than 2^31 - 1 frames", what, e);
        const int64_t n = ms_frames(it.s0, it.s1, hop, frames_of(it.n_samples, hop));
        AVX_REQUIRE(n <= AVEXHIP_MEASURE_MAX_EVENT_FRAMES, "%s: event %d: %lld frames, more than %d", what, e, (long long)n, AVEXHIP_MEASURE_MAX_EVENT_FRAMES);
        AVX_REQUIRE((int64_t)it.n_frames == n && (int64_t)it.first_run == runs && it.env_offset == frames,
                    "%s: event %d: n_frames=%d first_run=%d env_offset=%lld, expected %lld, %lld and %lld", what, e, it.n_frames, it.first_run,
                    (long long)it.env_offset, (long long)n, (long long)runs, (long long)frames);
        frames += n;
        runs += (n + kMsRun - 1) / kMsRun;
        AVX_REQUIRE(frames < ((int64_t)1 << 31) && runs < ((int64_t)1 << 31), "%s: more than 2^31 - 1 frames", what);
    }
    AVX_REQUIRE(total_frames == frames && total_runs == runs, "%s: total_frames=%lld total_runs=%lld, the table holds %lld and %lld", what,
                (long long)total_frames, (long long)total_runs, (long long)frames, (long long)runs);
    return AVEXHIP_OK;
}

}  // namespace

extern "C" size_t avexhip_measure_partials_bytes(int64_t n_runs) {
    if (n_runs < 0 || n_runs >= ((int64_t)1 << 31)) return 0;
    return (size_t)n_runs * kMsPartWords * sizeof(float);
}

extern "C" int avexhip_measure_frames(const float* wav_dev, int64_t wav_samples, const avexhip_measure_event* ev_host, const avexhip_measure_event* ev_dev,
                                      int n_events, int hop, const float* tables_dev, int64_t total_frames, int64_t total_runs, void* partials_dev,
                                      size_t partials_bytes, float* envelope_dev, void* stream) {
    AVX_REQUIRE(n_events >= 0, "measure_frames: n_events=%d", n_events);
    if (n_events == 0) return AVEXHIP_OK;                        // no event at all
    AVX_REQUIRE(wav_dev && tables_dev, "measure_frames: null argument");
    AVX_REQUIRE(aligned(wav_dev, 16) && aligned(tables_dev, 16) && aligned(partials_dev, 4) && aligned(envelope_dev, 4),
                "measure_frames: wav_dev and tables_dev must be 16-byte aligned, partials_dev and envelope_dev 4-byte aligned");
    AVX_REQUIRE(wav_samples >= 1, "measure_frames: wav_samples=%lld", (long long)wav_samples);
    AVXH_TRY(measure_events_check("measure_frames", ev_host, ev_dev, n_events, hop, wav_samples, -1, total_frames, total_runs));
    if (total_runs == 0) return AVEXHIP_OK;                      // no event holds a frame
    AVX_REQUIRE(partials_dev && envelope_dev, "measure_frames: null argument");
    AVXH_TRY(partials_check("measure_frames", partials_bytes, total_runs, avexhip_measure_partials_bytes(total_runs)));
    hipLaunchKernelGGL(measure_frames_kernel, dim3((unsigned)total_runs), dim3(256), 0, (hipStream_t)stream, wav_dev, ev_dev, n_events, hop, tables_dev,
                       (float*)partials_dev, envelope_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_measure_reduce(const avexhip_measure_event* ev_host, const avexhip_measure_event* ev_dev, int n_events, int hop, int64_t total_frames,
                                      int64_t total_runs, const void* partials_dev, size_t partials_bytes, const float* envelope_dev, const float* noise_dev,
                                      int n_rec, double q_lo, double q_c, double q_hi, float* spectrum_dev, const avexhip_measure_result* out, void* stream) {
    AVX_REQUIRE(n_events >= 0, "measure_reduce: n_events=%d", n_events);
    if (n_events == 0) return AVEXHIP_OK;
    AVX_REQUIRE(out && spectrum_dev, "measure_reduce: null argument");
    AVX_REQUIRE(q_lo > 0.0 && q_lo <= q_c && q_c <= q_hi && q_hi < 1.0, "measure_reduce: quantile levels %g, %g, %g: 0 < q_lo <= q_c <= q_hi < 1 expected", q_lo, q_c,
                q_hi);
    AVX_REQUIRE(noise_dev ? n_rec >= 1 : true, "measure_reduce: n_rec=%d rows of noise", n_rec);
    const void* cols4[] = {out->n_frames, out->nonfinite, out->low_bin, out->centre_bin, out->high_bin, out->peak_bin, out->low_frame, out->centre_frame,
                           out->high_frame, out->peak_frame};
    for (const void* p : cols4) AVX_REQUIRE(p && aligned(p, 4), "measure_reduce: a null or misaligned result column");
    AVX_REQUIRE(out->energy && out->snr_db && aligned(out->energy, 8) && aligned(out->snr_db, 8), "measure_reduce: a null or misaligned result column");
    AVX_REQUIRE(aligned(partials_dev, 4) && aligned(envelope_dev, 4) && aligned(noise_dev, 4) && aligned(spectrum_dev, 4),
                "measure_reduce: the device arrays must be 4-byte aligned");
    AVXH_TRY(measure_events_check("measure_reduce", ev_host, ev_dev, n_events, hop, -1, noise_dev ? n_rec : -1, total_frames, total_runs));
    AVX_REQUIRE(total_runs == 0 || (partials_dev && envelope_dev), "measure_reduce: null argument");
    AVXH_TRY(partials_check("measure_reduce", partials_bytes, total_runs, avexhip_measure_partials_bytes(total_runs)));
    hipLaunchKernelGGL(measure_reduce_kernel, dim3((unsigned)n_events), dim3(256), 0, (hipStream_t)stream, ev_dev, hop, (const float*)partials_dev, envelope_dev,
                       noise_dev, q_lo, q_c, q_hi, spectrum_dev, *out);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
