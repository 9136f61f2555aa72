// Audio ingest on the device: PCM samples as the file holds them -> mono float32 -> the model's sample rate.
//
// The reference decodes on the host (soundfile / torchaudio.load), averages channels (`noise_wav.mean(dim=0)`,
// avex/data/augmentations.py:269-271; `audio_stereo_to_mono(..., "average")`, birdset_train_splits.py:186) and resamples with
// `torchaudio.transforms.Resample(orig, new)` (augmentations.py:274-276) -- torchaudio's documented band-limited sinc interpolation
// (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99; optionally Kaiser-windowed), restated here:
//   orig, new reduced by their gcd;  base = min(orig, new) * rolloff;  width = ceil(lowpass_width * orig / base)
//   kernel[p][j] = sinc(t) * window(t) * base / orig,   t = ((j - width) / orig - p / new) * base  clamped to +-lowpass_width
//   out[q * new + p] = sum_j kernel[p][j] * x[q * orig + j - width]   (zero outside the clip),   length ceil(new * T / orig)
// PARITY UNPINNED against torchaudio (absent from both machines); the checker is oracle/ingest_oracle.py.
//
// Every arithmetic chain is written once and called by the per-file kernel and by the batched one, which is what makes a row of
// avexhip_ingest_batch the bits of the per-file path: pcm_mono_sample (decode, channel mean), sinc_stage + sinc_taps (the polyphase
// filter), interp_wings (resampy's two filter wings).  The kernels differ in which inputs a workgroup stages and in what lies behind a
// clip's end.  A plan is one ResamplePlan, read by avexhip_resample_forward on the host and, by value in a table, by the batched kernels.
#include <math.h>

#include <vector>

#include "common.h"

namespace {

// Frame i of interleaved PCM [frames][channels] of the given sample format -> one mono fp32 sample (the channels added in channel order,
// then divided by their number), normalised like soundfile / torchaudio do for float32 output: int16 / 32768, int24 / 2^23, int32 / 2^31,
// uint8 (x - 128) / 128; fmt 0 is float32, 64 float64.  `bad` collects non-finite float samples.
__device__ __forceinline__ float pcm_mono_sample(const unsigned char* __restrict__ raw, int fmt, int channels, int64_t i, bool& bad) {
    float acc = 0.f;
    for (int c = 0; c < channels; ++c) {
        const int64_t e = i * channels + c;
        float v;
        if (fmt == 16) v = (float)((const short*)raw)[e] * (1.0f / 32768.0f);
        else if (fmt == 32) v = (float)((const int*)raw)[e] * (1.0f / 2147483648.0f);
        else if (fmt == 24) {
            const unsigned char* p = raw + 3 * e;
            int s = (int)p[0] | ((int)p[1] << 8) | ((int)(signed char)p[2] << 16);
            v = (float)s * (1.0f / 8388608.0f);
        } else if (fmt == 8) v = ((float)raw[e] - 128.0f) * (1.0f / 128.0f);
        else {
            v = fmt == 64 ? (float)((const double*)raw)[e] : ((const float*)raw)[e];
            bad |= non_finite(v);
        }
        acc += v;
    }
    return channels > 1 ? acc / (float)channels : acc;
}

__global__ __launch_bounds__(256) void pcm_to_mono_kernel(const unsigned char* __restrict__ raw, int fmt, int channels, int64_t frames, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= frames) return;
    bool bad = false;                                           // (not reported here: a NaN stays a NaN in the output)
    out[i] = pcm_mono_sample(raw, fmt, channels, i, bad);
}

// The polyphase sinc filter.  sinc_stage: xs[s] = input sample first + s for s < span, zero outside [lo, hi) (src[k] = sample k of the
// clip; 256 threads, the caller's barrier follows).  sinc_taps: one output from its table row and its `taps` staged inputs, one fmaf chain.
__device__ __forceinline__ void sinc_stage(float* xs, int span, int64_t first, const float* __restrict__ src, int64_t lo, int64_t hi) {
    for (int s = threadIdx.x; s < span; s += 256) {
        const int64_t k = first + s;
        xs[s] = (k >= lo && k < hi) ? src[k] : 0.f;
    }
}
__device__ __forceinline__ float sinc_taps(const float* __restrict__ row, const float* xin, int taps) {
    float acc = 0.f;
    for (int j = 0; j < taps; ++j) acc = __builtin_fmaf(row[j], xin[j], acc);
    return acc;
}

// One workgroup = 256 consecutive output samples of one clip.  The input samples they touch are staged in LDS; the polyphase table
// [new][taps] is read through the caches (each output reads one row).
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, int64_t T, int64_t x_stride, const float* __restrict__ table, int orig, int newr,
                                                       int width, int taps, float* __restrict__ out, int64_t n_out, int64_t out_stride) {
    extern __shared__ float xs[];
    const int b = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * 256;
    const int64_t q0 = i0 / newr, q1 = (i0 + 255) / newr;
    const int64_t lo = q0 * orig - width;                       // first input sample any of the 256 outputs reads
    const int span = (int)((q1 - q0) * orig) + taps;
    sinc_stage(xs, span, lo, x + (int64_t)b * x_stride, 0, T);
    __syncthreads();
    const int64_t i = i0 + threadIdx.x;
    if (i >= n_out) return;
    const int64_t q = i / newr;
    const int p = (int)(i - q * newr);
    out[(int64_t)b * out_stride + i] = sinc_taps(table + (int64_t)p * taps, xs + (int)((q - q0) * orig), taps);
}

// resampy's interpolating resampler (librosa.resample(..., res_type="kaiser_best"), birdset_train_splits.py:190-196): output sample t sits
// at input time t / ratio; its two filter wings walk a half-window table (64 zero crossings x 512 samples each, Kaiser-windowed sinc)
// in steps of scale * 512 entries, every weight linearly interpolated between neighbouring table entries.  One thread per output
// sample; table and input through the caches (the table is 128 KB, a wing touches every index_step-th entry of it).
// interp_wings: output sample t of a clip of T samples at src, before the scaling by `post`.
__device__ __forceinline__ float interp_wings(const float* __restrict__ src, int64_t T, int64_t t, const float* __restrict__ win, const float* __restrict__ delta,
                                              int nwin, int num_table, int index_step, double scale, double time_increment) {
    float acc = 0.f;
    const double time_register = (double)t * time_increment;
    const int64_t n = (int64_t)time_register;
    double frac = scale * (time_register - (double)n);
    double index_frac = frac * num_table;
    int offset = (int)index_frac;
    float eta = (float)(index_frac - offset);
    int64_t i_max = (nwin - offset) / index_step;
    i_max = i_max < n + 1 ? i_max : n + 1;
    for (int64_t i = 0; i < i_max; ++i) {
        const int k = offset + (int)i * index_step;
        acc = __builtin_fmaf(__builtin_fmaf(eta, delta[k], win[k]), src[n - i], acc);
    }
    frac = scale - frac;
    index_frac = frac * num_table;
    offset = (int)index_frac;
    eta = (float)(index_frac - offset);
    int64_t k_max = (nwin - offset) / index_step;
    k_max = k_max < T - n - 1 ? k_max : T - n - 1;
    for (int64_t k = 0; k < k_max; ++k) {
        const int q = offset + (int)k * index_step;
        acc = __builtin_fmaf(__builtin_fmaf(eta, delta[q], win[q]), src[n + k + 1], acc);
    }
    return acc;
}

__global__ __launch_bounds__(256) void resample_interp_kernel(const float* __restrict__ x, int64_t T, int64_t x_stride, const float* __restrict__ win,
                                                              const float* __restrict__ delta, int nwin, int num_table, int index_step, double scale,
                                                              double time_increment, int64_t n_res, float post, float* __restrict__ out, int64_t n_out,
                                                              int64_t out_stride) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_out) return;
    const int b = blockIdx.y;
    float acc = 0.f;
    // librosa's fix_length zero-fills beyond resampy's int(T * ratio) samples
    if (t < n_res) acc = interp_wings(x + (int64_t)b * x_stride, T, t, win, delta, nwin, num_table, index_step, scale, time_increment);
    out[(int64_t)b * out_stride + t] = acc * post;
}

int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// the modified Bessel function I0 by its power series, at most max_terms terms
double bessel_i0(double z, int max_terms) {
    double s = 1.0, t = 1.0;
    for (int k = 1; k < max_terms; ++k) { t *= (z / (2.0 * k)) * (z / (2.0 * k)); s += t; if (t < 1e-18 * s) break; }
    return s;
}

// a plan as host and device read it
struct ResamplePlan {
    float* table = nullptr;                    // device memory, owned by the avexhip_resample_plan
    int orig = 0, newr = 0, width = 0, taps = 0;                 // sinc plans
    int interp = 0, nwin = 0, num_table = 0, index_step = 0;     // interpolating (resampy) plans: table = [win | delta], each nwin floats
    double scale = 1.0, time_increment = 1.0, ratio = 1.0;
    float post = 1.f;
};

}  // namespace

struct avexhip_resample_plan { ResamplePlan d; };

extern "C" avexhip_resample_plan* avexhip_resample_plan_create(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, double kaiser_beta) {
    if (orig_freq <= 0 || new_freq <= 0 || lowpass_filter_width <= 0 || !(rolloff > 0.0 && rolloff <= 1.0)) {
        avexhip_set_error("resample_plan_create: bad arguments orig=%d new=%d width=%d rolloff=%g", orig_freq, new_freq, lowpass_filter_width, rolloff);
        return nullptr;
    }
    const int g = gcd_i(orig_freq, new_freq);
    const int orig = orig_freq / g, newr = new_freq / g;
    const double base = (double)(orig < newr ? orig : newr) * rolloff;
    const int width = (int)ceil((double)lowpass_filter_width * orig / base);
    const int taps = 2 * width + orig;
    if ((int64_t)newr * taps > (1 << 26) || taps + 256 / newr * orig + 2 * orig > 36000) {
        avexhip_set_error("resample_plan_create: %d -> %d Hz reduces to %d -> %d (%d taps): table or staging too large", orig_freq, new_freq, orig, newr, taps);
        return nullptr;
    }
    std::vector<float> tab((size_t)newr * taps);
    const double lpw = (double)lowpass_filter_width;
    for (int p = 0; p < newr; ++p)
        for (int j = 0; j < taps; ++j) {
            double t = ((double)(j - width) / orig - (double)p / newr) * base;
            t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
            double w;
            if (kaiser_beta > 0.0) { const double r = t / lpw; w = bessel_i0(kaiser_beta * sqrt(1.0 - r * r), 64) / bessel_i0(kaiser_beta, 64); }
            else { const double c = cos(t * M_PI / lpw / 2.0); w = c * c; }
            const double a = t * M_PI;
            const double sinc = a == 0.0 ? 1.0 : sin(a) / a;
            tab[(size_t)p * taps + j] = (float)(sinc * w * base / orig);
        }
    avexhip_resample_plan* pl = new avexhip_resample_plan();
    pl->d.orig = orig; pl->d.newr = newr; pl->d.width = width; pl->d.taps = taps;
    if (hipMalloc((void**)&pl->d.table, sizeof(float) * tab.size()) != hipSuccess ||
        hipMemcpy(pl->d.table, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
        avexhip_set_error("resample_plan_create: device allocation failed");
        avexhip_resample_plan_destroy(pl);
        return nullptr;
    }
    return pl;
}

extern "C" avexhip_resample_plan* avexhip_resample_interp_plan_create(int orig_freq, int new_freq, int num_zeros, int precision, double rolloff,
                                                                       double kaiser_beta, int scale_energy) {
    if (orig_freq <= 0 || new_freq <= 0 || num_zeros <= 0 || num_zeros > 256 || precision < 1 || precision > 12 || !(rolloff > 0.0 && rolloff <= 1.0) ||
        !(kaiser_beta >= 0.0)) {
        avexhip_set_error("resample_interp_plan_create: bad arguments orig=%d new=%d zeros=%d precision=%d rolloff=%g beta=%g", orig_freq, new_freq, num_zeros,
                          precision, rolloff, kaiser_beta);
        return nullptr;
    }
    // resampy.filters.sinc_window: half of a Kaiser-windowed sinc on num_zeros * 2^precision + 1 points
    const int num_bits = 1 << precision;
    const int n = num_bits * num_zeros;
    const double ratio = (double)new_freq / (double)orig_freq;
    std::vector<double> w((size_t)n + 1);
    const double i0b = bessel_i0(kaiser_beta, 256);
    for (int i = 0; i <= n; ++i) {
        const double a = rolloff * (double)num_zeros * (double)i / (double)n;       // rolloff * linspace(0, num_zeros, n + 1)
        const double sinc = a == 0.0 ? 1.0 : sin(M_PI * a) / (M_PI * a);
        const double r = (double)i / (double)n;                                      // kaiser(2 n + 1)[n + i]
        const double taper = bessel_i0(kaiser_beta * sqrt(1.0 - r * r), 256) / i0b;
        w[i] = rolloff * sinc * taper * (ratio < 1.0 ? ratio : 1.0);                 // resampy scales the window when it decimates
    }
    std::vector<float> tab(2 * ((size_t)n + 1));
    for (int i = 0; i <= n; ++i) {
        tab[i] = (float)w[i];
        tab[(size_t)n + 1 + i] = i < n ? (float)(w[i + 1] - w[i]) : 0.f;
    }
    avexhip_resample_plan* pl = new avexhip_resample_plan();
    ResamplePlan& d = pl->d;
    d.interp = 1; d.orig = orig_freq; d.newr = new_freq; d.nwin = n + 1; d.num_table = num_bits;
    d.ratio = ratio; d.time_increment = 1.0 / ratio; d.scale = ratio < 1.0 ? ratio : 1.0;
    d.index_step = (int)(d.scale * num_bits);
    d.post = scale_energy ? (float)(1.0 / sqrt(ratio)) : 1.f;
    if (d.index_step < 1 || hipMalloc((void**)&d.table, sizeof(float) * tab.size()) != hipSuccess ||
        hipMemcpy(d.table, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
        avexhip_set_error("resample_interp_plan_create: %d -> %d Hz: ratio too small for the table, or device allocation failed", orig_freq, new_freq);
        avexhip_resample_plan_destroy(pl);
        return nullptr;
    }
    return pl;
}

extern "C" void avexhip_resample_plan_destroy(avexhip_resample_plan* p) {
    if (!p) return;
    if (p->d.table) (void)hipFree(p->d.table);
    delete p;
}

extern "C" int64_t avexhip_resample_out_length(const avexhip_resample_plan* p, int64_t T) {
    if (!p || T <= 0) return 0;
    if (p->d.interp) return (int64_t)ceil((double)T * p->d.ratio);      // librosa: n_samples = ceil(len * ratio), resampy's int(len * ratio) zero-padded up to it
    return ((int64_t)p->d.newr * T + p->d.orig - 1) / p->d.orig;
}

// bytes of LDS a workgroup of a sinc plan stages at most
static size_t sinc_lds_bytes(const ResamplePlan& d) { return sizeof(float) * (size_t)((256 / d.newr + 2) * d.orig + d.taps); }

extern "C" int avexhip_resample_forward(const avexhip_resample_plan* pl, const float* x_dev, int B, int64_t T, int64_t x_stride, float* out_dev,
                                        int64_t out_stride, void* stream) {
    AVX_REQUIRE(pl && x_dev && out_dev, "resample_forward: null argument");
    AVX_REQUIRE(B > 0 && T > 0 && B <= 65535, "resample_forward: bad shape B=%d T=%lld", B, (long long)T);
    const ResamplePlan* p = &pl->d;
    const int64_t n_out = avexhip_resample_out_length(pl, T);
    if (x_stride <= 0) x_stride = T;
    if (out_stride <= 0) out_stride = n_out;
    AVX_REQUIRE(B == 1 || x_stride >= T, "resample_forward: x_stride %lld < %lld input samples (rows would overlap)", (long long)x_stride, (long long)T);
    AVX_REQUIRE(out_stride >= n_out, "resample_forward: out_stride %lld < %lld output samples", (long long)out_stride, (long long)n_out);
    if (p->interp) {
        const int64_t n_res = (int64_t)((double)T * p->ratio);
        hipLaunchKernelGGL(resample_interp_kernel, dim3((unsigned)((n_out + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, x_dev, T, x_stride, p->table,
                           p->table + p->nwin, p->nwin, p->num_table, p->index_step, p->scale, p->time_increment, n_res, p->post, out_dev, n_out, out_stride);
        AVX_LAUNCH_CHECK();
        return AVEXHIP_OK;
    }
    AVX_ENSURE_LDS(resample_kernel, 160 * 1024);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((n_out + 255) / 256), B), dim3(256), sinc_lds_bytes(*p), (hipStream_t)stream, x_dev, T, x_stride, p->table, p->orig,
                       p->newr, p->width, p->taps, out_dev, n_out, out_stride);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

extern "C" int avexhip_pcm_to_mono_f32(const void* raw_dev, int sample_format, int channels, int64_t frames, float* out_dev, void* stream) {
    AVX_REQUIRE(raw_dev && out_dev, "pcm_to_mono_f32: null argument");
    AVX_REQUIRE(channels > 0 && channels <= 64 && frames > 0, "pcm_to_mono_f32: bad shape channels=%d frames=%lld", channels, (long long)frames);
    AVX_REQUIRE(sample_format == 0 || sample_format == 8 || sample_format == 16 || sample_format == 24 || sample_format == 32 || sample_format == 64,
                "pcm_to_mono_f32: sample_format %d (0 = float32, 64 = float64, 8 / 16 / 24 / 32 = integer PCM)", sample_format);
    hipLaunchKernelGGL(pcm_to_mono_kernel, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)raw_dev, sample_format,
                       channels, frames, out_dev);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// Batched ingest: B clips of any format / channel count / rate / length -> the padded model batch, in a fixed number of launches.
// What the reference's Collater makes on the host (avex/data/dataset.py:256-399 on avex/data/audio_utils.py:16-73): channel mean,
// clips with a NaN / Inf replaced by zeros, a window of the clip or zero padding up to the model length, the padding mask.
//   ingest_mono_kernel      every item's raw samples -> mono fp32, only the input span its window (and the filter halo) reads;
//                           float payloads are scanned whole for NaN / Inf (flag per item)
//   ingest_resample_kernel  row b, sample j = sample start_b + j of the item's full-clip resampling (sinc_stage + sinc_taps or
//                           interp_wings, the calls resample_kernel / resample_interp_kernel make: the same bits), zeros behind
//                           `valid`, the mask, zero rows for flagged items
// ------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int kIngestMaxPlans = 16;
constexpr int kIngestMonoBlocks = 64;          // blocks per item in the mono stage; each walks its item's chunks with this stride

struct IngestPlanTable { ResamplePlan p[kIngestMaxPlans]; };

__host__ __device__ inline int ingest_sample_bytes(int fmt) { return fmt == 8 ? 1 : fmt == 16 ? 2 : fmt == 24 ? 3 : fmt == 64 ? 8 : 4; }

// [lo, hi): the mono samples of a clip of T frames that the outputs start .. start + valid - 1 of its resampling read (pl == nullptr:
// the clip is at the target rate already).  The same integer / double arithmetic as the kernels, so host and device agree.
__host__ __device__ inline void ingest_span(const ResamplePlan* pl, int64_t T, int64_t start, int64_t valid, int64_t* lo, int64_t* hi) {
    int64_t a = 0, b = 0;
    if (valid > 0) {
        const int64_t last = start + valid - 1;
        if (!pl) { a = start; b = last + 1; }
        else if (!pl->interp) {
            a = (start / pl->newr) * pl->orig - pl->width;
            b = (last / pl->newr) * pl->orig - pl->width + pl->taps;
        } else {
            const int64_t n_res = (int64_t)((double)T * pl->ratio);
            const int64_t t1 = last < n_res - 1 ? last : n_res - 1;
            if (t1 >= start) {
                const int64_t wing = pl->nwin / pl->index_step + 1;      // a wing reads at most (nwin - offset) / index_step samples
                a = (int64_t)((double)start * pl->time_increment) - wing;
                b = (int64_t)((double)t1 * pl->time_increment) + wing + 1;
            }
        }
        a = a < 0 ? 0 : a;
        b = b > T ? T : b;
        if (b < a) b = a;
    }
    *lo = a; *hi = b;
}

// grid (kIngestMonoBlocks, B).  Integer PCM: the span only.  Float payloads: the whole clip (the NaN / Inf test covers every sample the
// reference's Collater would see), stores inside the span only.
__global__ __launch_bounds__(256) void ingest_mono_kernel(const unsigned char* __restrict__ raw, const avexhip_ingest_item* __restrict__ items,
                                                          IngestPlanTable plans, float* __restrict__ ws, int64_t ws_stride, int* __restrict__ flags) {
    const int b = blockIdx.y;
    const avexhip_ingest_item it = items[b];
    int64_t lo, hi;
    ingest_span(it.plan >= 0 ? &plans.p[it.plan] : nullptr, it.frames, it.start, it.valid, &lo, &hi);
    const bool is_float = it.sample_format == 0 || it.sample_format == 64;
    const int64_t first = is_float ? 0 : lo, end = is_float ? it.frames : hi;
    const unsigned char* src = raw + it.offset;
    float* dst = ws + (int64_t)b * ws_stride;
    bool bad = false;
    for (int64_t i = first + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)kIngestMonoBlocks * 256) {
        const float v = pcm_mono_sample(src, it.sample_format, it.channels, i, bad);
        if (i >= lo && i < hi) dst[i - lo] = v;
    }
    if (bad) flags[b] = 1;                     // every writer stores the same value
}

// grid (ceil(T_out / 256), B): one workgroup = 256 consecutive samples of one output row.
__global__ __launch_bounds__(256) void ingest_resample_kernel(const avexhip_ingest_item* __restrict__ items, IngestPlanTable plans, const float* __restrict__ ws,
                                                              int64_t ws_stride, const int* __restrict__ flags, float* __restrict__ out, int64_t out_stride,
                                                              unsigned char* __restrict__ mask, int64_t T_out) {
    extern __shared__ float xs[];
    const int b = blockIdx.y;
    const avexhip_ingest_item it = items[b];
    const int64_t j0 = (int64_t)blockIdx.x * 256, j = j0 + threadIdx.x;
    const int64_t valid = it.valid;
    float acc = 0.f;
    if (j0 < valid && flags[b] == 0) {                              // workgroup-uniform
        const ResamplePlan* pl = it.plan >= 0 ? &plans.p[it.plan] : nullptr;
        int64_t lo, hi;
        ingest_span(pl, it.frames, it.start, valid, &lo, &hi);
        const float* src = ws + (int64_t)b * ws_stride - lo;        // src[k] = mono sample k of the clip, for lo <= k < hi
        const int64_t T = it.frames;
        if (!pl) {
            if (j < valid) acc = src[it.start + j];
        } else if (!pl->interp) {
            const int orig = pl->orig, newr = pl->newr, taps = pl->taps;
            const int64_t i0 = it.start + j0;
            const int64_t ilast = it.start + (j0 + 255 < valid - 1 ? j0 + 255 : valid - 1);
            const int64_t q0 = i0 / newr, q1 = ilast / newr;
            const int64_t first = q0 * orig - pl->width;             // first input sample any of the workgroup's outputs reads
            const int span = (int)((q1 - q0) * orig) + taps;
            sinc_stage(xs, span, first, src, lo, hi);                // [lo, hi) is what [0, T) holds of the reads: zero outside, as resample_kernel
            __syncthreads();
            if (j < valid) {
                const int64_t i = it.start + j;
                const int64_t q = i / newr;
                const int p = (int)(i - q * newr);
                acc = sinc_taps(pl->table + (int64_t)p * taps, xs + (int)((q - q0) * orig), taps);
            }
        } else if (j < valid) {
            const int64_t t = it.start + j;
            const int64_t n_res = (int64_t)((double)T * pl->ratio);
            if (t < n_res)
                acc = interp_wings(src, T, t, pl->table, pl->table + pl->nwin, pl->nwin, pl->num_table, pl->index_step, pl->scale, pl->time_increment);
            acc = acc * pl->post;
        }
    }
    if (j < T_out) {
        out[(int64_t)b * out_stride + j] = acc;                      // acc is still 0 behind `valid` and in flagged rows
        mask[(int64_t)b * T_out + j] = j >= valid ? 1 : 0;
    }
}

// everything avexhip_ingest_batch_workspace_bytes / avexhip_ingest_batch check, and the layout they share
struct IngestLayout { IngestPlanTable table; int64_t ws_stride; size_t flag_bytes, total_bytes, lds_bytes; };

int ingest_layout(const avexhip_ingest_item* items, int B, const avexhip_resample_plan* const* plans, int n_plans, int64_t T_out, size_t raw_bytes,
                  bool check_raw, IngestLayout* L) {
    AVX_REQUIRE(items, "ingest_batch: null item list");
    AVX_REQUIRE(B >= 1 && B <= 65535, "ingest_batch: B=%d outside 1..65535", B);
    AVX_REQUIRE(T_out >= 1 && T_out <= ((int64_t)1 << 31) - 256, "ingest_batch: T_out=%lld", (long long)T_out);
    AVX_REQUIRE(n_plans >= 0 && n_plans <= kIngestMaxPlans && (n_plans == 0 || plans), "ingest_batch: %d resample plans (at most %d per batch)", n_plans,
                kIngestMaxPlans);
    memset(&L->table, 0, sizeof(L->table));
    size_t lds = 0;
    for (int i = 0; i < n_plans; ++i) {
        const avexhip_resample_plan* p = plans[i];
        AVX_REQUIRE(p && p->d.table, "ingest_batch: plan %d is null", i);
        L->table.p[i] = p->d;
        const size_t need = p->d.interp ? 0 : sinc_lds_bytes(p->d);
        lds = need > lds ? need : lds;
    }
    int64_t stride = 1;
    for (int b = 0; b < B; ++b) {
        const avexhip_ingest_item& it = items[b];
        const int f = it.sample_format;
        AVX_REQUIRE(f == 0 || f == 8 || f == 16 || f == 24 || f == 32 || f == 64, "ingest_batch: item %d: sample_format %d", b, f);
        AVX_REQUIRE(it.channels > 0 && it.channels <= 64 && it.frames > 0 && it.frames <= ((int64_t)1 << 40), "ingest_batch: item %d: channels=%d frames=%lld", b,
                    it.channels, (long long)it.frames);
        AVX_REQUIRE(it.plan >= -1 && it.plan < n_plans, "ingest_batch: item %d: plan index %d outside -1..%d", b, it.plan, n_plans - 1);
        AVX_REQUIRE(it.valid >= 0 && it.valid <= T_out, "ingest_batch: item %d: valid=%lld outside 0..T_out=%lld", b, (long long)it.valid, (long long)T_out);
        const int64_t n_out = it.plan < 0 ? it.frames : avexhip_resample_out_length(plans[it.plan], it.frames);
        AVX_REQUIRE(it.start >= 0 && it.start <= n_out - it.valid, "ingest_batch: item %d: window %lld + %lld leaves the clip's %lld resampled samples", b,
                    (long long)it.start, (long long)it.valid, (long long)n_out);
        if (check_raw) {
            const uint64_t bytes = (uint64_t)it.frames * (uint64_t)it.channels * (uint64_t)ingest_sample_bytes(f);
            AVX_REQUIRE(it.offset >= 0 && it.offset % 8 == 0, "ingest_batch: item %d: byte offset %lld is not a non-negative multiple of 8", b, (long long)it.offset);
            AVX_REQUIRE((uint64_t)it.offset <= raw_bytes && bytes <= raw_bytes - (uint64_t)it.offset, "ingest_batch: item %d: %llu bytes at offset %lld leave the %llu-byte buffer",
                        b, (unsigned long long)bytes, (long long)it.offset, (unsigned long long)raw_bytes);
        }
        int64_t lo, hi;
        ingest_span(it.plan >= 0 ? &L->table.p[it.plan] : nullptr, it.frames, it.start, it.valid, &lo, &hi);
        stride = hi - lo > stride ? hi - lo : stride;
    }
    L->ws_stride = (stride + 3) & ~(int64_t)3;
    L->flag_bytes = ((size_t)B * sizeof(int) + 255) & ~(size_t)255;
    L->total_bytes = L->flag_bytes + (size_t)B * (size_t)L->ws_stride * sizeof(float);
    L->lds_bytes = lds;
    return AVEXHIP_OK;
}

}  // namespace

extern "C" size_t avexhip_ingest_batch_workspace_bytes(const avexhip_ingest_item* items_host, int B, const avexhip_resample_plan* const* plans, int n_plans,
                                                       int64_t T_out) {
    IngestLayout L;
    if (ingest_layout(items_host, B, plans, n_plans, T_out, 0, false, &L) != AVEXHIP_OK) return 0;
    return L.total_bytes;
}

extern "C" int avexhip_ingest_batch(const void* raw_dev, size_t raw_bytes, const avexhip_ingest_item* items_host, const avexhip_ingest_item* items_dev, int B,
                                    const avexhip_resample_plan* const* plans, int n_plans, int64_t T_out, float* wav_dev, int64_t wav_stride,
                                    uint8_t* mask_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    AVX_REQUIRE(raw_dev && items_dev && wav_dev && mask_dev && workspace_dev, "ingest_batch: null argument");
    AVX_REQUIRE(((uintptr_t)raw_dev & 7) == 0 && ((uintptr_t)items_dev & 7) == 0 && ((uintptr_t)workspace_dev & 15) == 0,
                "ingest_batch: raw_dev / items_dev must be 8-byte aligned, workspace_dev 16-byte aligned");
    IngestLayout L;
    AVXH_TRY(ingest_layout(items_host, B, plans, n_plans, T_out, raw_bytes, true, &L));
    if (wav_stride <= 0) wav_stride = T_out;
    AVX_REQUIRE(wav_stride >= T_out, "ingest_batch: wav_stride %lld < T_out %lld", (long long)wav_stride, (long long)T_out);
    if (workspace_bytes < L.total_bytes) {
        avexhip_set_error("ingest_batch: workspace of %llu bytes, %llu needed (avexhip_ingest_batch_workspace_bytes)", (unsigned long long)workspace_bytes,
                          (unsigned long long)L.total_bytes);
        return AVEXHIP_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    int* flags = (int*)workspace_dev;
    float* ws = (float*)((char*)workspace_dev + L.flag_bytes);
    AVX_HIP_CHECK(hipMemsetAsync(flags, 0, L.flag_bytes, s));
    hipLaunchKernelGGL(ingest_mono_kernel, dim3(kIngestMonoBlocks, B), dim3(256), 0, s, (const unsigned char*)raw_dev, items_dev, L.table, ws, L.ws_stride, flags);
    AVX_LAUNCH_CHECK();
    AVX_ENSURE_LDS(ingest_resample_kernel, 160 * 1024);
    hipLaunchKernelGGL(ingest_resample_kernel, dim3((unsigned)((T_out + 255) / 256), B), dim3(256), L.lds_bytes, s, items_dev, L.table, ws, L.ws_stride, flags,
                       wav_dev, wav_stride, mask_dev, T_out);
    AVX_LAUNCH_CHECK();
    return AVEXHIP_OK;
}
