// The walk over the 512-sample frames of resident recordings, shared by activity_frames_kernel (activity.hip) and, through
// frame_power.h, the kernels of soundscape.hip, measure.hip and regions.hip; windows.hip takes the recording refusal alone.
//
// CONTRACT.  A recording is `n_samples` samples of one 16-byte aligned fp32 buffer from sample `base` on; it has frames_of(n_samples,
// hop) frames, frame f its samples [f hop, f hop + 512), no padding.  The frames, and whatever a kernel counts in them (workgroups,
// segments, runs), lie back to back over a device table of recordings, each row with the number of its first one; a workgroup finds its
// row with last_at_most.  stage_span brings the samples of consecutive frames of ONE recording to LDS and never reads outside
// [r_lo, r_hi): the entry points refuse, on the host and before any launch, a recording that leaves the buffer (recording_check), so every
// read is at base + j with j < n_samples inside the buffer.  stage_span and stage_twiddles assume 256 threads and contain NO barrier: the
// caller places its own before the span or the twiddles are read (and before a span that is still being read is staged again).
//
// Nothing here includes fft512.h, so a file that needs the walk or the refusals alone stays out of build.py's EXTRA_FLAGS.  Windowing,
// the transform and the power of ONE frame per wave are frame_power.h's; activity_frames_kernel packs a pair and keeps its own.  The
// host side also holds what the table checks of the four files open with (table_check) and the refusal of a short buffer of run
// partials (partials_check): one text each.
#pragma once
#include "common.h"

namespace {

constexpr int kRecFrame = 512;                   // n_fft, fixed
constexpr int kRecBins = 257;

__host__ __device__ __forceinline__ int64_t frames_of(int64_t n_samples, int hop) { return n_samples < kRecFrame ? 0 : (n_samples - kRecFrame) / hop + 1; }

// the last of n rows whose key(row) is <= i, for keys that do not decrease: rows that hold nothing share their successor's key, and the
// last of them is the one that does
template <typename Key>
__device__ __forceinline__ int last_at_most(int n, int i, Key key) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key(mid) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// wav[s0 .. s0 + len) -> span[lead .. lead + len), lead = s0 % 4 (returned): 16 bytes per lane wherever a whole aligned chunk lies inside
// the recording [r_lo, r_hi), single loads and zeros elsewhere.  span: 16-byte aligned LDS of at least lead + len floats rounded up to 4.
__device__ __forceinline__ int stage_span(float* span, const float* __restrict__ wav, int64_t s0, int len, int64_t r_lo, int64_t r_hi) {
    const int64_t a0 = s0 & ~(int64_t)3;                         // wav is 16-byte aligned (checked on the host)
    const int lead = (int)(s0 - a0);
    len += lead;
    for (int c = threadIdx.x * 4; c < len; c += 256 * 4) {
        const int64_t i = a0 + c;
        f32x4 q;
        if (i >= r_lo && i + 4 <= r_hi) {
            q = *(const f32x4*)(wav + i);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = (i + e >= r_lo && i + e < r_hi) ? wav[i + e] : 0.f;
        }
        *(f32x4*)(span + c) = q;
    }
    return lead;
}

// tables: [512] window, then [512] (cos, -sin)(2 pi k / 512); the second half -> tw[512]
__device__ __forceinline__ void stage_twiddles(float2* tw, const float* __restrict__ tables) {
    const float2* twg = (const float2*)(tables + kRecFrame);
    tw[threadIdx.x] = twg[threadIdx.x];
    tw[threadIdx.x + 256] = twg[threadIdx.x + 256];
}

// ---- what the entry points refuse, on the host -----------------------------------------------------------------------------------------
// A recording that is empty, starts in front of the buffer or (wav_samples >= 0: there is a buffer to check) ends behind it.  `window`: the
// row is a window that carries its recording's base and length, and is refused in one sentence.
inline int recording_check(const char* what, int row, int64_t n_samples, int64_t base, int64_t wav_samples, bool window = false) {
    const bool holds = n_samples >= 1 && base >= 0, fits = wav_samples < 0 || base <= wav_samples - n_samples;
    if (window) {
        AVX_REQUIRE(holds && fits, "%s: window %d: a recording of %lld samples at %lld leaves the buffer's %lld samples", what, row, (long long)n_samples,
                    (long long)base, (long long)wav_samples);
        return AVEXHIP_OK;
    }
    AVX_REQUIRE(holds, "%s: recording %d: %lld samples at %lld", what, row, (long long)n_samples, (long long)base);
    AVX_REQUIRE(fits, "%s: recording %d: %lld samples at %lld leave the buffer's %lld samples", what, row, (long long)n_samples, (long long)base,
                (long long)wav_samples);
    return AVEXHIP_OK;
}

inline int hop_check(const char* what, int hop) {
    AVX_REQUIRE(hop >= AVEXHIP_ACTIVITY_MIN_HOP && hop <= kRecFrame, "%s: hop=%d outside %d..%d", what, hop, AVEXHIP_ACTIVITY_MIN_HOP, kRecFrame);
    return AVEXHIP_OK;
}

// The first refusals of every table check, in this order: a null table, a device table off its 8 bytes (`dev_name` names it), fewer than
// one row (`need_rows`: false where the caller has returned for an empty table before), a hop outside its range.  The walk over the
// rows stays with the caller: what it counts differs (blocks, segments and runs, runs, events).
inline int table_check(const char* what, const void* host, const void* dev, const char* dev_name, int n_rec, bool need_rows, int hop) {
    AVX_REQUIRE(host && dev, "%s: null argument", what);
    AVX_REQUIRE(aligned(dev, 8), "%s: %s must be 8-byte aligned", what, dev_name);
    AVX_REQUIRE(!need_rows || n_rec >= 1, "%s: n_rec=%d", what, n_rec);
    return hop_check(what, hop);
}

// a buffer of run partials that is too small for the table's runs
inline int partials_check(const char* what, size_t have, int64_t runs, size_t need) {
    if (have >= need) return AVEXHIP_OK;
    avexhip_set_error("%s: partials_bytes=%zu, %lld runs need %zu", what, have, (long long)runs, need);
    return AVEXHIP_ERR_WORKSPACE;
}

// bins lo .. hi - 1 of the band `name`, or `name number` with number >= 0
inline int bin_band_check(const char* what, const char* name, int number, int lo, int hi) {
    if (lo >= 0 && lo < hi && hi <= kRecBins) return AVEXHIP_OK;
    if (number >= 0) avexhip_set_error("%s: %s %d: bins %d..%d outside 0 <= lo < hi <= %d", what, name, number, lo, hi, kRecBins);
    else avexhip_set_error("%s: %s: bins %d..%d outside 0 <= lo < hi <= %d", what, name, lo, hi, kRecBins);
    return AVEXHIP_ERR_INVALID;
}

}  // namespace
