// Whole-recording windows (ABI 14): every sliding window of a recording from ONE resident fp32 waveform -- what load_audio leaves on the
// device: decoded, mono, resampled once -- instead of one ingest per window.
//
// The reference crops a long clip to a single window (pad_or_window, avex/data/audio_utils.py:16-73) and reserves a name for the step
// that would say which windows are worth embedding (avex/preprocessing/activity_detector.py, an empty file; activity.hip builds it on the
// table and the statistics of this file).  A window row here is
// pad_or_window(wav[start:], window_len, "start"): the samples, then zeros, padding_mask True on the zeros.
//   window_stats_kernel    per window: max |x| (fp32) and sum x^2 (fp64) over its valid samples
//   window_select_kernel   flags from two thresholds -> the kept window numbers in increasing order and their count (prefix sum, no atomics)
//   window_gather_kernel   rows and masks of a list (or a contiguous range) of windows, one launch
// All three read a device table of avexhip_window (recording base, start, valid), so windows of several recordings share a launch.
// Every read is at base + start + j with j < valid, and the entry points refuse a table for which that leaves the recording, or whose
// recording leaves the buffer (recording_check, rec_frames.h: the refusal activity.hip and soundscape.hip make of theirs).
#include <math.h>

#include "block_prims.h"
#include "common.h"
#include "rec_frames.h"

namespace {

constexpr int kWinThreads = 256;
constexpr int kWinStep = kWinThreads * 4;        // samples one pass of a workgroup covers: thread t holds samples 4 t .. 4 t + 3 of it
constexpr int kSelectThreads = 1024;

// One workgroup per window.  Sample j of the window belongs to thread (j / 4) % 256, slot j % 4, pass j / 1024; a slot adds its squares
// in pass order, a thread adds its slots as (0 + 1) + (2 + 3), a wave its lanes by a butterfly, thread 0 the waves as (0 + 1) + (2 + 3).
// Nothing in that order looks at another window or at where the window sits in memory: the wide loads (16 bytes per lane where the
// window's first sample is 16-byte aligned) and the scalar ones feed the same sums.  The zeros a partial last pass adds change no bit
// (every square is >= +0).
__global__ __launch_bounds__(kWinThreads) void window_stats_kernel(const float* __restrict__ wav, const avexhip_window* __restrict__ win,
                                                                   double* __restrict__ energy, float* __restrict__ peak) {
    __shared__ double wave_sum_d[kWinThreads / 64];
    __shared__ float wave_max_f[kWinThreads / 64];
    const int w = blockIdx.x;
    const avexhip_window it = win[w];
    const int valid = it.valid;
    const float* src = wav + it.base + it.start;
    const bool wide = ((it.base + it.start) & 3) == 0;           // wav is 16-byte aligned (checked on the host): so is this window's first sample
    const int full = valid / kWinStep;                           // passes in which every thread holds four valid samples
    const float* p = src + threadIdx.x * 4;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float mx = 0.f;
    bool bad = false;
    auto see = [&](const float (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] += (double)v[e] * (double)v[e];               // the product of two fp32 values is exact in fp64
            mx = __builtin_fmaxf(mx, __builtin_fabsf(v[e]));
            bad |= non_finite(v[e]);
        }
    };
    if (wide) {
#pragma unroll 4
        for (int k = 0; k < full; ++k) {
            const f32x4 q = *(const f32x4*)(p + (int64_t)k * kWinStep);
            const float v[4] = {q[0], q[1], q[2], q[3]};
            see(v);
        }
    } else {
#pragma unroll 4
        for (int k = 0; k < full; ++k) {
            const float* q = p + (int64_t)k * kWinStep;
            const float v[4] = {q[0], q[1], q[2], q[3]};
            see(v);
        }
    }
    const int j0 = full * kWinStep + threadIdx.x * 4;
    if (j0 < valid) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = j0 + e < valid ? src[j0 + e] : 0.f;
        see(v);
    }
    const double s = wave_reduce((acc[0] + acc[1]) + (acc[2] + acc[3]), BlockSum());
    mx = wave_max(mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { wave_sum_d[wave] = s; wave_max_f[wave] = mx; }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) {
        const double e = (wave_sum_d[0] + wave_sum_d[1]) + (wave_sum_d[2] + wave_sum_d[3]);
        const float m = __builtin_fmaxf(__builtin_fmaxf(wave_max_f[0], wave_max_f[1]), __builtin_fmaxf(wave_max_f[2], wave_max_f[3]));
        energy[w] = any_bad ? (double)NAN : e;
        peak[w] = any_bad ? NAN : m;
    }
}

// One workgroup walks the table 1024 windows at a time (block_compact, block_prims.h): a kept window's position is the number of kept
// windows in front of it, so the list is in increasing order whatever the timing.  The table is 32 bytes and the statistics 12 bytes per
// window; an hour at a 1 s hop is 3 600 windows.
__global__ __launch_bounds__(kSelectThreads) void window_select_kernel(const avexhip_window* __restrict__ win, const double* __restrict__ energy,
                                                                       const float* __restrict__ peak, int n_win, double thr_energy, float thr_peak,
                                                                       int* __restrict__ kept, int* __restrict__ count) {
    block_compact<kSelectThreads>(n_win, [&](int i) {
        const int valid = win[i].valid;
        return valid > 0 && energy[i] >= thr_energy * (double)valid && peak[i] >= thr_peak;      // a NaN fails both compares
    }, kept, count);
}

// grid (ceil(window_len / 1024), B): a thread owns four consecutive samples of one row and their mask bytes.  Window starts are
// arbitrary, so a 16-byte load is taken only in rows whose first sample is 16-byte aligned (row-uniform) and only for four valid
// samples; 16-byte stores and 4-byte mask stores only where the host found every row aligned (wide_out / wide_mask).
__global__ __launch_bounds__(kWinThreads) void window_gather_kernel(const float* __restrict__ wav, const avexhip_window* __restrict__ win, int n_win,
                                                                    const int* __restrict__ index, int first, int window_len, float* __restrict__ out,
                                                                    int64_t out_stride, unsigned char* __restrict__ mask, int wide_out, int wide_mask) {
    const int b = blockIdx.y;
    const int j0 = (blockIdx.x * kWinThreads + threadIdx.x) * 4;
    if (j0 >= window_len) return;
    const int w = index ? index[b] : first + b;
    int valid = 0;
    const float* src = wav;
    bool wide_src = false;
    if (w >= 0 && w < n_win) {                                   // a number from a device list the host never saw: outside the table, an empty row
        const avexhip_window it = win[w];
        valid = it.valid;
        src = wav + it.base + it.start;
        wide_src = ((it.base + it.start) & 3) == 0;
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (wide_src && j0 + 4 <= valid) {
        const f32x4 q = *(const f32x4*)(src + j0);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j0 + e < valid) v[e] = src[j0 + e];
    }
    float* o = out + (int64_t)b * out_stride + j0;
    unsigned char* m = mask + (int64_t)b * window_len + j0;
    if (j0 + 4 <= window_len) {
        if (wide_out) *(f32x4*)o = (f32x4){v[0], v[1], v[2], v[3]};
        else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; }
        if (wide_mask) {
            *(uint32_t*)m = (j0 >= valid ? 0x1u : 0u) | (j0 + 1 >= valid ? 0x100u : 0u) | (j0 + 2 >= valid ? 0x10000u : 0u) | (j0 + 3 >= valid ? 0x1000000u : 0u);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = j0 + e >= valid ? 1 : 0;
        }
    } else {
        for (int e = 0; j0 + e < window_len; ++e) {
            o[e] = v[e];
            m[e] = j0 + e >= valid ? 1 : 0;
        }
    }
}

// what stats and gather refuse, for the windows lo .. hi - 1 of the table
int windows_check(const char* what, const float* wav_dev, int64_t wav_samples, const avexhip_window* win_host, const avexhip_window* win_dev, int n_win,
                  int window_len, int lo, int hi) {
    AVX_REQUIRE(wav_dev && win_host && win_dev, "%s: null argument", what);
    AVX_REQUIRE(aligned(wav_dev, 16) && aligned(win_dev, 8), "%s: wav_dev must be 16-byte aligned, win_dev 8-byte aligned", what);
    AVX_REQUIRE(n_win >= 1, "%s: n_win=%d", what, n_win);
    AVX_REQUIRE(window_len >= 1 && window_len <= (1 << 30), "%s: window_len=%d outside 1..2^30", what, window_len);
    AVX_REQUIRE(wav_samples >= 1, "%s: wav_samples=%lld", what, (long long)wav_samples);
    for (int w = lo; w < hi; ++w) {
        const avexhip_window& it = win_host[w];
        AVXH_TRY(recording_check(what, w, it.n_samples, it.base, wav_samples, true));
        AVX_REQUIRE(it.valid >= 0 && it.valid <= window_len, "%s: window %d: valid=%d outside 0..window_len=%d", what, w, it.valid, window_len);
        AVX_REQUIRE(it.start >= 0 && it.start <= it.n_samples - it.valid, "%s: window %d: %lld + %d leaves the recording's %lld samples", what, w,
                    (long long)it.start, it.valid, (long long)it.n_samples);
    }
    return AVEXHIP_OK;
}

}  // namespace

extern "C" int avexhip_window_stats(const float* wav_dev, int64_t wav_samples, const avexhip_window* win_host, const avexhip_window* win_dev, int n_win,
                                    int window_len, double* energy_dev, float* peak_dev, void* stream) {
    AVX_REQUIRE(energy_dev && peak_dev, "window_stats: null argument");
    AVXH_TRY(windows_check("window_stats", wav_dev, wav_samples, win_host, win_dev, n_win, window_len, 0, n_win));
    hipLaunchKernelGGL(window_stats_kernel, dim3((unsigned)n_win), dim3(kWinThreads), 0, (hipStream_t)stream, wav_dev, win_dev, energy_dev, peak_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_window_select(const avexhip_window* win_dev, const double* energy_dev, const float* peak_dev, int n_win, double thr_energy,
                                     float thr_peak, int32_t* kept_dev, int32_t* count_dev, void* stream) {
    AVX_REQUIRE(win_dev && energy_dev && peak_dev && kept_dev && count_dev, "window_select: null argument");
    AVX_REQUIRE(aligned(win_dev, 8), "window_select: win_dev must be 8-byte aligned");
    AVX_REQUIRE(n_win >= 1, "window_select: n_win=%d", n_win);
    AVX_REQUIRE(!(thr_energy != thr_energy) && !(thr_peak != thr_peak), "window_select: a threshold is NaN (-inf turns one off)");
    hipLaunchKernelGGL(window_select_kernel, dim3(1), dim3(kSelectThreads), 0, (hipStream_t)stream, win_dev, energy_dev, peak_dev, n_win, thr_energy, thr_peak,
                       kept_dev, count_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_window_gather(const float* wav_dev, int64_t wav_samples, const avexhip_window* win_host, const avexhip_window* win_dev, int n_win,
                                     const int32_t* index_dev, int first, int B, int window_len, float* out_dev, int64_t out_stride, uint8_t* mask_dev,
                                     void* stream) {
    AVX_REQUIRE(out_dev && mask_dev, "window_gather: null argument");
    AVX_REQUIRE(B >= 1 && B <= 65535, "window_gather: B=%d outside 1..65535", B);
    AVX_REQUIRE(index_dev || (first >= 0 && n_win >= 1 && first <= n_win - B), "window_gather: windows %d .. %d leave the table's %d", first, first + B - 1, n_win);
    AVXH_TRY(windows_check("window_gather", wav_dev, wav_samples, win_host, win_dev, n_win, window_len, index_dev ? 0 : first, index_dev ? n_win : first + B));
    if (out_stride <= 0) out_stride = window_len;
    AVX_REQUIRE(out_stride >= window_len, "window_gather: out_stride %lld < window_len %d", (long long)out_stride, window_len);
    const int wide_out = aligned(out_dev, 16) && out_stride % 4 == 0;
    const int wide_mask = aligned(mask_dev, 4) && window_len % 4 == 0;
    hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)((window_len + kWinStep - 1) / kWinStep), B), dim3(kWinThreads), 0, (hipStream_t)stream, wav_dev,
                       win_dev, n_win, index_dev, first, window_len, out_dev, out_stride, mask_dev, wide_out, wide_mask);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
