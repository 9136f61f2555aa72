// Acoustic indices over recordings (ABI 23): per segment of `segment_frames` frames the long-term spectrum and what the standard
// soundscape indices are made of, from the resident waveform of windows.hip and the frames of activity.hip (512 samples every `hop`,
// periodic Hann, no padding).
//   soundscape_stats_kernel    a run of up to 64 consecutive frames of ONE segment per workgroup: |X|^2 per frame and bin, and per bin
//                              the sums of P, of A = sqrt(P), of |A[t] - A[t-1]| and the count of P > thr, added in frame order; one
//                              partial row per run (with the run's first and last amplitude row); the frame's total power on the side
//   soundscape_reduce_kernel   per (segment, bin) the runs' partials in run order, |first A of a run - last A of the run before| between
//                              them (the same bits the runs computed), the divisions -> mean_power, mean_amplitude, abs_diff, count_above
//   soundscape_indices_kernel  one workgroup per segment, fp64: ACI, ADI, AEI, BI, NDSI, Hf, Ht, H from those fp32 statistics
// The power row is wave_frame_power (frame_power.h, shared with measure.hip and regions.hip): fft512_wave with ONE frame per wave and a
// zero imaginary part, not activity_frames_kernel's pair packing: a frame's P[t, :] is then a function of its own 512 samples (packed
// beside a loud frame, a quiet one's bins carry the partner's rounding noise, eps * |X_loud|; for per-bin amplitudes that is not
// tolerable).  A frame of zeros gives +0 in every bin by arithmetic alone; a frame that holds a NaN or an Inf is set to NaN in every bin.
// No atomics, sums in one fixed order: the same bits on every run and in any company.  The walk over the frames is activity.hip's
// (rec_frames.h: the frame count, the recording of a run or a segment, the span and twiddle staging, the refusals of a table, a
// recording, a hop, a bin band and a short buffer of partials); every partial row, statistic row and frame index follows from the
// checked table.
#include <math.h>

#include "block_prims.h"
#include "common.h"
#include "frame_power.h"

namespace {

constexpr int kSsRun = AVEXHIP_SOUNDSCAPE_RUN_FRAMES;            // frames per workgroup of the stats kernel
// a partial row, in 4-byte words: the four sums, the first and the last amplitude row of the run, the run's non-finite frames
constexpr int kPartPow = 0, kPartAmp = kRecBins, kPartDiff = 2 * kRecBins, kPartCount = 3 * kRecBins, kPartFirst = 4 * kRecBins, kPartLast = 5 * kRecBins,
              kPartBad = 6 * kRecBins, kPartWords = 6 * kRecBins + 2;

__host__ __device__ __forceinline__ int ss_runs_per_segment(int S) { return (S + kSsRun - 1) / kSsRun; }

// grid: one workgroup per run (avexhip_soundscape_recording::first_run numbers them), 256 threads.  tables: [512] window, then [512]
// (cos, -sin)(2 pi k / 512).  LDS: 8 224 + 18 432 + 4 096 + 4 160 + 16 bytes = 34 928.
__global__ __launch_bounds__(256) void soundscape_stats_kernel(const float* __restrict__ wav, const avexhip_soundscape_recording* __restrict__ rec, int n_rec,
                                                               int hop, int S, float thr, const float* __restrict__ tables, float* __restrict__ partials,
                                                               float* __restrict__ frame_power) {
    const FramePowerLds lds = frame_power_lds();
    __shared__ float prow[kFpStep][kFpPRow];
    __shared__ int bad_of[kFpStep];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = last_at_most(n_rec, (int)blockIdx.x, [&](int i) { return rec[i].first_run; });
    const avexhip_soundscape_recording it = rec[r];
    const int64_t F = frames_of(it.n_samples, hop);
    const int per_seg = ss_runs_per_segment(S);
    const int run = (int)blockIdx.x - it.first_run;
    const int64_t seg = run / per_seg;
    const int in_seg = (run % per_seg) * kSsRun;                 // the run's first frame, counted inside its segment
    if (seg * S >= F) return;                                    // (block-uniform; the entry point launches no such workgroup)
    const int64_t seg_n = F - seg * S < S ? F - seg * S : S;
    if (in_seg >= seg_n) return;
    const int nf = seg_n - in_seg < kSsRun ? (int)(seg_n - in_seg) : kSsRun;
    const int64_t f0 = seg * S + in_seg;                         // the run's first frame, counted inside its recording

    stage_twiddles(lds.tw, tables);

    // thread t owns bin t; thread 0 bin 256 as well
    const int n_own = tid == 0 ? 2 : 1;
    float s_pow[2] = {0.f, 0.f}, s_amp[2] = {0.f, 0.f}, s_diff[2] = {0.f, 0.f}, a_first[2] = {0.f, 0.f}, a_prev[2] = {0.f, 0.f};
    int s_cnt[2] = {0, 0}, n_bad = 0;

    const int64_t r_lo = it.base, r_hi = it.base + it.n_samples;
    for (int st = 0; st < nf; st += kFpStep) {                   // (block-uniform trip count)
        const int ns = nf - st < kFpStep ? nf - st : kFpStep;
        __syncthreads();                                         // the step before has read span and prow
        // ---- the span of the step's frames -> LDS: lead <= 3, (ns - 1) hop + 512 <= 3 * 512 + 512 ---------------------------------------
        const int lead = stage_span(lds.span, wav, it.base + (f0 + st) * hop, (ns - 1) * hop + kRecFrame, r_lo, r_hi);
        __syncthreads();

        if (wave < ns) {                                         // (wave-uniform; only wave syncs inside)
            // A lane adds its bins in increasing order, the wave its lanes by a butterfly: a fixed order, the same for every launch.
            float total = 0.f;
            const bool bad = wave_frame_power(lds.span + lead + wave * hop, tables, lds.zbuf[wave], lds.tw, lane, [&](int, int k, float p) {
                prow[wave][k] = p;
                total += p;
            });
            total = wave_sum(total);
            if (lane == 0) {
                frame_power[it.first_frame + f0 + st + wave] = total;
                bad_of[wave] = bad ? 1 : 0;
            }
        }
        __syncthreads();

        // ---- the step's frames into the bin owners' sums, in frame order ------------------------------------------------------------------
        for (int j = 0; j < ns; ++j) {
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                if (o < n_own) {
                    const float p = prow[j][o == 0 ? tid : 256];
                    const float a = sqrtf(p);
                    s_pow[o] += p;
                    s_amp[o] += a;
                    if (st + j == 0) a_first[o] = a; else s_diff[o] += fabsf(a - a_prev[o]);
                    a_prev[o] = a;
                    s_cnt[o] += p > thr ? 1 : 0;                 // false for a NaN
                }
            }
            if (tid == 0) n_bad += bad_of[j];
        }
    }

    float* part = partials + (int64_t)blockIdx.x * kPartWords;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        if (o < n_own) {
            const int k = o == 0 ? tid : 256;
            part[kPartPow + k] = s_pow[o];
            part[kPartAmp + k] = s_amp[o];
            part[kPartDiff + k] = s_diff[o];
            ((int*)part)[kPartCount + k] = s_cnt[o];
            part[kPartFirst + k] = a_first[o];
            part[kPartLast + k] = a_prev[o];
        }
    }
    if (tid == 0) ((int*)part)[kPartBad] = n_bad;
}

// what the reduce and the indices kernels need to know of segment g
struct SsSegment {
    int64_t first_frame;         // counted over all recordings
    int n, first_run, n_runs;
};
__device__ __forceinline__ SsSegment ss_segment_of(const avexhip_soundscape_recording* __restrict__ rec, int n_rec, int hop, int S, int g) {
    const int r = last_at_most(n_rec, g, [&](int i) { return rec[i].first_segment; });
    const avexhip_soundscape_recording it = rec[r];
    const int64_t F = frames_of(it.n_samples, hop);
    const int64_t gl = g - it.first_segment;
    SsSegment s;
    const int64_t left = F - gl * S;
    s.n = left < S ? (int)left : S;
    s.first_frame = it.first_frame + gl * S;
    s.first_run = it.first_run + (int)gl * ss_runs_per_segment(S);
    s.n_runs = (s.n + kSsRun - 1) / kSsRun;
    return s;
}

// grid: one workgroup per segment, 256 threads; thread t reduces bin t, thread 0 bin 256 as well and the non-finite count.
__global__ __launch_bounds__(256) void soundscape_reduce_kernel(const avexhip_soundscape_recording* __restrict__ rec, int n_rec, int hop, int S,
                                                                const float* __restrict__ partials, float* __restrict__ mean_power,
                                                                float* __restrict__ mean_amplitude, float* __restrict__ abs_diff,
                                                                int* __restrict__ count_above, int* __restrict__ nonfinite) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const SsSegment sg = ss_segment_of(rec, n_rec, hop, S, g);
    if (sg.n <= 0) return;                                       // (the entry point launches no such workgroup)
    const float* part0 = partials + (int64_t)sg.first_run * kPartWords;
    int n_bad = 0;
    for (int u = 0; u < sg.n_runs; ++u) n_bad += ((const int*)(part0 + (int64_t)u * kPartWords))[kPartBad];      // (every thread: the NaN rule below)
    if (tid == 0) nonfinite[g] = n_bad;
    const float n = (float)sg.n;                                 // exact: S <= 2^24
    for (int k = tid; k < kRecBins; k += 256) {
        float s_pow = 0.f, s_amp = 0.f, s_diff = 0.f, last = 0.f;
        int cnt = 0;
        for (int u = 0; u < sg.n_runs; ++u) {
            const float* part = part0 + (int64_t)u * kPartWords;
            s_pow += part[kPartPow + k];
            s_amp += part[kPartAmp + k];
            if (u > 0) s_diff += fabsf(part[kPartFirst + k] - last);
            s_diff += part[kPartDiff + k];
            last = part[kPartLast + k];
            cnt += ((const int*)part)[kPartCount + k];
        }
        const int64_t o = (int64_t)g * kRecBins + k;
        mean_power[o] = n_bad ? NAN : s_pow / n;
        mean_amplitude[o] = n_bad ? NAN : s_amp / n;
        abs_diff[o] = n_bad ? NAN : s_diff;
        count_above[o] = cnt;
    }
}

// grid: one workgroup per segment, 256 threads.  Every sum: a thread adds its own terms in increasing order, block_scan the threads in
// thread order.  out: [G, 8] fp64 in the order of AVEXHIP_SOUNDSCAPE_INDICES.
__global__ __launch_bounds__(256) void soundscape_indices_kernel(const avexhip_soundscape_recording* __restrict__ rec, int n_rec, int hop, int S,
                                                                 avexhip_soundscape_index_spec spec, const float* __restrict__ mean_power,
                                                                 const float* __restrict__ mean_amplitude, const float* __restrict__ abs_diff,
                                                                 const int* __restrict__ count_above, const int* __restrict__ nonfinite,
                                                                 const float* __restrict__ frame_power, double* __restrict__ out) {
    __shared__ double wt[4];
    __shared__ double p_adi[AVEXHIP_SOUNDSCAPE_MAX_ADI_BANDS], row_adi[AVEXHIP_SOUNDSCAPE_MAX_ADI_BANDS];
    const int g = blockIdx.x, tid = threadIdx.x;
    const SsSegment sg = ss_segment_of(rec, n_rec, hop, S, g);
    if (sg.n <= 0) return;
    double* dst = out + (int64_t)g * AVEXHIP_SOUNDSCAPE_INDICES;
    if (nonfinite[g] > 0) {                                      // (block-uniform)
        if (tid < AVEXHIP_SOUNDSCAPE_INDICES) dst[tid] = NAN;
        return;
    }
    const float* mp = mean_power + (int64_t)g * kRecBins;
    const float* ma = mean_amplitude + (int64_t)g * kRecBins;
    const float* ad = abs_diff + (int64_t)g * kRecBins;
    const int* ca = count_above + (int64_t)g * kRecBins;
    const double n = (double)sg.n;
    const double full_scale = (double)AVEXHIP_SOUNDSCAPE_FULL_SCALE;
    auto block_sum = [&](double v) {
        double excl, total;
        block_scan<4>(v, 0.0, BlockSum(), wt, &excl, &total);
        return total;
    };
    auto within = [](int k, const int32_t (&b)[2]) { return k >= b[0] && k < b[1]; };

    // ---- aci, ndsi, the spectrum's total, the quietest bin of bio_band ---------------------------------------------------------------
    double v_aci = 0.0, v_bio = 0.0, v_anthro = 0.0, v_band = 0.0, v_min = INFINITY;
    for (int k = tid; k < kRecBins; k += 256) {
        const double p = (double)mp[k], a = (double)ma[k];
        if (within(k, spec.band)) {
            v_aci += a == 0.0 ? 0.0 : (double)ad[k] / (n * a);
            v_band += p;
        }
        if (within(k, spec.bio)) {
            v_bio += p;
            const double floor_p = 1e-12 * full_scale;
            const double L = 10.0 * log10((p > floor_p ? p : floor_p) / full_scale);
            v_min = L < v_min ? L : v_min;
        }
        if (within(k, spec.anthro)) v_anthro += p;
    }
    const double aci = block_sum(v_aci), bio = block_sum(v_bio), anthro = block_sum(v_anthro), band = block_sum(v_band);
    double excl, l_min;
    block_scan<4>(v_min, (double)INFINITY, BlockMin(), wt, &excl, &l_min);

    // ---- bi, hf -----------------------------------------------------------------------------------------------------------------------
    double v_bi = 0.0, v_hf = 0.0;
    for (int k = tid; k < kRecBins; k += 256) {
        const double p = (double)mp[k];
        if (within(k, spec.bio)) {
            const double floor_p = 1e-12 * full_scale;
            v_bi += 10.0 * log10((p > floor_p ? p : floor_p) / full_scale) - l_min;
        }
        if (within(k, spec.band) && band > 0.0) {
            const double q = p / band;
            v_hf += q > 0.0 ? q * log(q) : 0.0;
        }
    }
    const double bi = block_sum(v_bi) * spec.bin_khz;
    const int K = spec.band[1] - spec.band[0];
    const double hf_sum = block_sum(v_hf);
    const double hf = (band > 0.0 && K >= 2) ? -hf_sum / log((double)K) : (double)NAN;

    // ---- ht over the segment's frames ---------------------------------------------------------------------------------------------------
    const float* fp = frame_power + sg.first_frame;
    double v_t = 0.0;
    for (int t = tid; t < sg.n; t += 256) v_t += (double)fp[t];
    const double t_total = block_sum(v_t);
    double v_ht = 0.0;
    if (t_total > 0.0) {
        for (int t = tid; t < sg.n; t += 256) {
            const double q = (double)fp[t] / t_total;
            v_ht += q > 0.0 ? q * log(q) : 0.0;
        }
    }
    const double ht_sum = block_sum(v_ht);
    const double ht = (t_total > 0.0 && sg.n >= 2) ? -ht_sum / log(n) : (double)NAN;

    // ---- adi, aei: thread j the occupancy of band j, thread i its row of |p_i - p_j|, thread 0 the sums in band order -------------------
    const int J = spec.n_adi;
    if (tid < J) {
        int c = 0;
        for (int k = spec.adi[tid][0]; k < spec.adi[tid][1]; ++k) c += ca[k];
        p_adi[tid] = (double)c / (n * (double)(spec.adi[tid][1] - spec.adi[tid][0]));
    }
    __syncthreads();
    if (tid < J) {
        double s = 0.0;
        for (int j = 0; j < J; ++j) s += fabs(p_adi[tid] - p_adi[j]);
        row_adi[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double sp = 0.0, gini = 0.0, ent = 0.0;
        for (int j = 0; j < J; ++j) sp += p_adi[j];
        for (int j = 0; j < J; ++j) {
            gini += row_adi[j];
            const double q = sp > 0.0 ? p_adi[j] / sp : 0.0;
            ent += q > 0.0 ? q * log(q) : 0.0;
        }
        dst[0] = aci;
        dst[1] = sp > 0.0 ? -ent : (double)NAN;
        dst[2] = sp > 0.0 ? gini / (2.0 * (double)J * sp) : (double)NAN;
        dst[3] = bi;
        dst[4] = bio + anthro == 0.0 ? (double)NAN : (bio - anthro) / (bio + anthro);
        dst[5] = hf;
        dst[6] = ht;
        dst[7] = hf * ht;
    }
}

// What every entry point refuses in the recording table; *runs_out = the workgroups of the stats kernel.  wav_samples < 0: no buffer to check.
int soundscape_recordings_check(const char* what, const avexhip_soundscape_recording* rec_host, const avexhip_soundscape_recording* rec_dev, int n_rec, int hop,
                                int S, int64_t wav_samples, int64_t total_frames, int64_t total_segments, int64_t* runs_out) {
    AVXH_TRY(table_check(what, rec_host, rec_dev, "rec_dev", n_rec, true, hop));
    AVX_REQUIRE(S >= 1 && S <= AVEXHIP_SOUNDSCAPE_MAX_SEGMENT_FRAMES, "%s: segment_frames=%d outside 1..%d", what, S, AVEXHIP_SOUNDSCAPE_MAX_SEGMENT_FRAMES);
    int64_t frames = 0, segments = 0, runs = 0;
    for (int r = 0; r < n_rec; ++r) {
        const avexhip_soundscape_recording& it = rec_host[r];
        AVXH_TRY(recording_check(what, r, it.n_samples, it.base, wav_samples));
        const int64_t F = frames_of(it.n_samples, hop);
        AVX_REQUIRE(it.first_frame == frames && (int64_t)it.first_segment == segments && (int64_t)it.first_run == runs,
                    "%s: recording %d: first_frame=%lld first_segment=%d first_run=%d, expected %lld, %lld and %lld", what, r, (long long)it.first_frame,
                    it.first_segment, it.first_run, (long long)frames, (long long)segments, (long long)runs);
        const int64_t whole = F / S, rest = F % S;
        frames += F;
        segments += whole + (rest ? 1 : 0);
        runs += whole * ss_runs_per_segment(S) + (rest + kSsRun - 1) / kSsRun;
        AVX_REQUIRE(frames < ((int64_t)1 << 31) && runs < ((int64_t)1 << 31), "%s: more than 2^31 - 1 frames", what);
    }
    AVX_REQUIRE(total_frames == frames && total_segments == segments, "%s: total_frames=%lld total_segments=%lld, the table holds %lld and %lld", what,
                (long long)total_frames, (long long)total_segments, (long long)frames, (long long)segments);
    if (runs_out) *runs_out = runs;
    return AVEXHIP_OK;
}

}  // namespace

extern "C" size_t avexhip_soundscape_partials_bytes(int64_t n_runs) {
    if (n_runs < 0 || n_runs >= ((int64_t)1 << 31)) return 0;
    return (size_t)n_runs * kPartWords * sizeof(float);
}

extern "C" int avexhip_soundscape_frames(const float* wav_dev, int64_t wav_samples, const avexhip_soundscape_recording* rec_host,
                                         const avexhip_soundscape_recording* rec_dev, int n_rec, int hop, int segment_frames, float threshold,
                                         const float* tables_dev, int64_t total_frames, int64_t total_segments, void* partials_dev, size_t partials_bytes,
                                         float* frame_power_dev, void* stream) {
    AVX_REQUIRE(wav_dev && tables_dev, "soundscape_frames: null argument");
    AVX_REQUIRE(aligned(wav_dev, 16) && aligned(tables_dev, 16) && aligned(partials_dev, 4) && aligned(frame_power_dev, 4),
                "soundscape_frames: wav_dev and tables_dev must be 16-byte aligned, partials_dev and frame_power_dev 4-byte aligned");
    AVX_REQUIRE(wav_samples >= 1, "soundscape_frames: wav_samples=%lld", (long long)wav_samples);
    AVX_REQUIRE(!(threshold != threshold) && threshold >= 0.f, "soundscape_frames: threshold=%g: a power >= 0 expected (not NaN; +inf counts no cell)", (double)threshold);
    int64_t runs = 0;
    AVXH_TRY(soundscape_recordings_check("soundscape_frames", rec_host, rec_dev, n_rec, hop, segment_frames, wav_samples, total_frames, total_segments, &runs));
    if (runs == 0) return AVEXHIP_OK;                            // no recording holds a frame
    AVX_REQUIRE(partials_dev && frame_power_dev, "soundscape_frames: null argument");
    AVXH_TRY(partials_check("soundscape_frames", partials_bytes, runs, avexhip_soundscape_partials_bytes(runs)));
    hipLaunchKernelGGL(soundscape_stats_kernel, dim3((unsigned)runs), dim3(256), 0, (hipStream_t)stream, wav_dev, rec_dev, n_rec, hop, segment_frames, threshold,
                       tables_dev, (float*)partials_dev, frame_power_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_soundscape_reduce(const avexhip_soundscape_recording* rec_host, const avexhip_soundscape_recording* rec_dev, int n_rec, int hop,
                                         int segment_frames, int64_t total_frames, int64_t total_segments, const void* partials_dev, size_t partials_bytes,
                                         float* mean_power_dev, float* mean_amplitude_dev, float* abs_diff_dev, int32_t* count_above_dev,
                                         int32_t* nonfinite_dev, void* stream) {
    AVX_REQUIRE(aligned(partials_dev, 4) && aligned(mean_power_dev, 4) && aligned(mean_amplitude_dev, 4) && aligned(abs_diff_dev, 4) &&
                    aligned(count_above_dev, 4) && aligned(nonfinite_dev, 4),
                "soundscape_reduce: the device arrays must be 4-byte aligned");
    int64_t runs = 0;
    AVXH_TRY(soundscape_recordings_check("soundscape_reduce", rec_host, rec_dev, n_rec, hop, segment_frames, -1, total_frames, total_segments, &runs));
    if (total_segments == 0) return AVEXHIP_OK;
    AVX_REQUIRE(partials_dev && mean_power_dev && mean_amplitude_dev && abs_diff_dev && count_above_dev && nonfinite_dev, "soundscape_reduce: null argument");
    AVXH_TRY(partials_check("soundscape_reduce", partials_bytes, runs, avexhip_soundscape_partials_bytes(runs)));
    hipLaunchKernelGGL(soundscape_reduce_kernel, dim3((unsigned)total_segments), dim3(256), 0, (hipStream_t)stream, rec_dev, n_rec, hop, segment_frames,
                       (const float*)partials_dev, mean_power_dev, mean_amplitude_dev, abs_diff_dev, count_above_dev, nonfinite_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_soundscape_indices(const avexhip_soundscape_recording* rec_host, const avexhip_soundscape_recording* rec_dev, int n_rec, int hop,
                                          int segment_frames, int64_t total_frames, int64_t total_segments, const avexhip_soundscape_index_spec* spec,
                                          const float* mean_power_dev, const float* mean_amplitude_dev, const float* abs_diff_dev,
                                          const int32_t* count_above_dev, const int32_t* nonfinite_dev, const float* frame_power_dev, double* indices_dev,
                                          void* stream) {
    AVX_REQUIRE(spec, "soundscape_indices: null argument");
    AVX_REQUIRE(aligned(mean_power_dev, 4) && aligned(mean_amplitude_dev, 4) && aligned(abs_diff_dev, 4) && aligned(count_above_dev, 4) &&
                    aligned(nonfinite_dev, 4) && aligned(frame_power_dev, 4) && aligned(indices_dev, 8),
                "soundscape_indices: indices_dev must be 8-byte aligned, the other device arrays 4-byte aligned");
    const struct { const char* name; const int32_t* b; } named[3] = {{"band", spec->band}, {"bio_band", spec->bio}, {"anthro_band", spec->anthro}};
    for (const auto& it : named) AVXH_TRY(bin_band_check("soundscape_indices", it.name, -1, it.b[0], it.b[1]));
    AVX_REQUIRE(spec->n_adi >= 1 && spec->n_adi <= AVEXHIP_SOUNDSCAPE_MAX_ADI_BANDS, "soundscape_indices: n_adi=%d outside 1..%d", spec->n_adi,
                AVEXHIP_SOUNDSCAPE_MAX_ADI_BANDS);
    for (int j = 0; j < spec->n_adi; ++j) AVXH_TRY(bin_band_check("soundscape_indices", "adi band", j, spec->adi[j][0], spec->adi[j][1]));
    AVX_REQUIRE(spec->bin_khz > 0.0 && spec->bin_khz < INFINITY, "soundscape_indices: bin_khz=%g: a finite width > 0 expected", spec->bin_khz);
    AVXH_TRY(soundscape_recordings_check("soundscape_indices", rec_host, rec_dev, n_rec, hop, segment_frames, -1, total_frames, total_segments, nullptr));
    if (total_segments == 0) return AVEXHIP_OK;
    AVX_REQUIRE(mean_power_dev && mean_amplitude_dev && abs_diff_dev && count_above_dev && nonfinite_dev && frame_power_dev && indices_dev,
                "soundscape_indices: null argument");
    hipLaunchKernelGGL(soundscape_indices_kernel, dim3((unsigned)total_segments), dim3(256), 0, (hipStream_t)stream, rec_dev, n_rec, hop, segment_frames, *spec,
                       mean_power_dev, mean_amplitude_dev, abs_diff_dev, count_above_dev, nonfinite_dev, frame_power_dev, indices_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
