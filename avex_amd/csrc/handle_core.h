// What the five encoder handles share (avexhip_beats in api.cpp; avexhip_eat / avexhip_aves / avexhip_stack in encoders.cpp;
// avexhip_effnet in effnet_handle.cpp).  All five: HandleBase (range alarm, profiling, the exported accessors' bodies), the argument
// checks of *_create / *_forward, the workspace Carver, the weight-table helpers and the tail of a forward.  The four transformer
// handles also: the frontend's window / mel bank, the positional-convolution packing, the per-layer parameter block, and the post-LN
// transformer layer loop on the GEMM / attention / LayerNorm kernels -- with the LayerNorms folded into the GEMM epilogues (GemmArgs)
// when the residual stream is kept in the operand type.
//
// The transformer encoders differ only in what surrounds the loop (frontend, positional scheme) and in four parameters of it:
//   alpha     DeepNorm residual scale (BEATs: (2 L)^(1/4), backbone.py:304-308; EAT, wav2vec2: 1)
//   eps       LayerNorm epsilon (BEATs / wav2vec2 1e-5, EAT 1e-6)
//   bias/gate relative-position bias table + gate (BEATs only)
//   hook site which raw GEMM output a layer's hook taps: fc2 (BEATs backbone.encoder.layers.{i}.fc2, AVES ...output_dense) or
//             the attention output projection (EAT backbone.model.blocks.{i}.attn.proj)
#pragma once
#include <math.h>
#include <stdlib.h>

#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace avxh {

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// hands out consecutive aligned pieces of a caller-provided workspace (NULL base: sizes only); `off` ends as the bytes needed
struct Carver {
    char* base;
    size_t off = 0;
    char* take(size_t bytes) { char* p = base ? base + off : nullptr; off += align_up(bytes); return p; }
};

struct StageRec {
    std::string name;
    double flops;
    hipEvent_t e0, e1;
};

// state every handle has: operand type, device allocations to free, the f16 range alarm, per-stage profiling
struct HandleBase {
    int dtype = AVEXHIP_F16;
    const char* who = "create";            // prefix of error messages
    std::vector<void*> allocs;
    // range alarm of the f16 conversions (GemmArgs::ovf): device counter every GEMM of a forward adds to, mirrored to pinned host
    // memory by an asynchronous copy at the end of each forward (read without a synchronisation by *_overflow_count)
    unsigned int* d_ovf = nullptr;
    unsigned int* h_ovf = nullptr;
    // log2(e) of the attention's exp2 folded into W_q / b_q in fp32 when the weights are packed (avx::attention's q_log2e): Q is rounded to the
    // operand type once and the scores are scaled by the exact 1/8.  AVEX_AMD_Q_LOG2E=0 keeps plain Q (the kernel then scales by a constant
    // it rounds to the operand type: 0.18 % off in bf16)
    bool q_log2e = !(getenv("AVEX_AMD_Q_LOG2E") && atoi(getenv("AVEX_AMD_Q_LOG2E")) == 0);
    bool profiling = false;
    std::vector<StageRec> recs;
    std::vector<std::string> prof_names;
    std::vector<const char*> prof_name_ptrs;
    std::vector<float> prof_ms;
    std::vector<double> prof_flops;

    int init_alarm() {
        if (hipMalloc((void**)&d_ovf, sizeof(unsigned int)) != hipSuccess || hipMemset(d_ovf, 0, sizeof(unsigned int)) != hipSuccess ||
            hipHostMalloc((void**)&h_ovf, sizeof(unsigned int), hipHostMallocDefault) != hipSuccess) {
            avexhip_set_error("%s: cannot allocate the range-alarm counter", who);
            return AVEXHIP_ERR_HIP;
        }
        *h_ovf = 0;
        return AVEXHIP_OK;
    }
    int mirror_alarm(hipStream_t s) {
        if (d_ovf && h_ovf) AVX_HIP_CHECK(hipMemcpyAsync(h_ovf, d_ovf, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        return AVEXHIP_OK;
    }
    // The bodies of the exported *_overflow_count / *_set_profiling / *_last_profile; `who` is the exported symbol's own message prefix
    // (BEATs' say "overflow_count", the later families' "eat_overflow_count").
    static int overflow_count(HandleBase* h, const char* who, uint32_t* events, void* sync_stream, int synchronize) {
        AVX_REQUIRE(h && events, "%s: null argument", who);
        if (synchronize) AVX_HIP_CHECK(hipStreamSynchronize((hipStream_t)sync_stream));
        *events = h->h_ovf ? *(volatile unsigned int*)h->h_ovf : 0u;
        return AVEXHIP_OK;
    }
    static int set_profiling(HandleBase* h, const char* who, int enabled) {
        AVX_REQUIRE(h, "%s: null handle", who);
        h->profiling = enabled != 0;
        return AVEXHIP_OK;
    }
    static int last_profile(const HandleBase* h, const char* who, const char* const** names, const float** ms, const double** flops, int* count) {
        AVX_REQUIRE(h && names && ms && flops && count, "%s: null argument", who);
        *names = h->prof_name_ptrs.data();
        *ms = h->prof_ms.data();
        *flops = h->prof_flops.data();
        *count = (int)h->prof_name_ptrs.size();
        return AVEXHIP_OK;
    }
    int overflow_reset(hipStream_t s) {
        AVX_HIP_CHECK(hipMemsetAsync(d_ovf, 0, sizeof(unsigned int), s));
        AVX_HIP_CHECK(hipMemcpyAsync(h_ovf, d_ovf, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        return AVEXHIP_OK;
    }
    // After the weights are packed and before any forward: the alarm counter holds what the UPLOAD clipped.  An f16 handle whose weights do
    // not fit the f16 range would compute with saturated weights, silently (the alarm of a forward only sees activations): refuse it.
    int weights_fit() {
        if (!d_ovf) return AVEXHIP_OK;
        unsigned int n = 0;
        AVX_HIP_CHECK(hipDeviceSynchronize());
        AVX_HIP_CHECK(hipMemcpy(&n, d_ovf, sizeof(n), hipMemcpyDeviceToHost));
        if (n != 0) {
            avexhip_set_error("%s: the checkpoint's weights do not fit the f16 range (+-65504): %u lane(s) clipped a value while packing them (a folded LayerNorm gain "
                              "or hidden_shift counts).  Use operand_dtype bf16 (fp32's exponent range).", who, n);
            return AVEXHIP_ERR_INVALID;
        }
        return AVEXHIP_OK;
    }
    virtual ~HandleBase() {
        for (void* p : allocs) (void)hipFree(p);
        if (d_ovf) (void)hipFree(d_ovf);
        if (h_ovf) (void)hipHostFree(h_ovf);
        for (auto& r : recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    }
};

// HIP events around every stage of a forward when the handle is in profiling mode
struct Prof {
    HandleBase* h;
    hipStream_t s;
    size_t next = 0;
    void begin(const char* name, double flops) {
        if (!h->profiling) return;
        if (next == h->recs.size()) {
            StageRec r;
            (void)hipEventCreate(&r.e0);
            (void)hipEventCreate(&r.e1);
            h->recs.push_back(r);
        }
        h->recs[next].name = name;
        h->recs[next].flops = flops;
        (void)hipEventRecord(h->recs[next].e0, s);
    }
    void end() {
        if (!h->profiling) return;
        (void)hipEventRecord(h->recs[next].e1, s);
        ++next;
    }
    // after the forward: aggregate by stage name (forces a stream synchronisation)
    int collect() {
        if (!h->profiling) return AVEXHIP_OK;
        AVX_HIP_CHECK(hipStreamSynchronize(s));
        std::map<std::string, std::pair<double, double>> agg;  // name -> (ms, flops)
        std::vector<std::string> order;
        for (size_t i = 0; i < next; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, h->recs[i].e0, h->recs[i].e1);
            if (!agg.count(h->recs[i].name)) order.push_back(h->recs[i].name);
            agg[h->recs[i].name].first += ms;
            agg[h->recs[i].name].second += h->recs[i].flops;
        }
        h->prof_names = order;
        h->prof_ms.clear(); h->prof_flops.clear(); h->prof_name_ptrs.clear();
        for (auto& nm : h->prof_names) {
            h->prof_ms.push_back((float)agg[nm].first);
            h->prof_flops.push_back(agg[nm].second);
        }
        for (auto& nm : h->prof_names) h->prof_name_ptrs.push_back(nm.c_str());
        return AVEXHIP_OK;
    }
};

// the tail of every forward: mirror the range alarm to the host, then (profiling mode only) read the events back
inline int finish_forward(HandleBase* h, Prof& prof, hipStream_t s) {
    AVXH_TRY(h->mirror_alarm(s));
    return prof.collect();
}

// GemmArgs of a product inside a forward: all zero but the handle's range alarm
inline void gemm_init(avx::GemmArgs& g, const HandleBase* h) {
    memset(&g, 0, sizeof(g));
    g.ovf = h->d_ovf;
}

// ---------------------------------------------------------------------------------------------
// Argument checks the families share; `who` is the entry point's message prefix ("eat_create", "aves_forward").  The *_create ones
// return false with the message set (a create returns NULL, not a code).  Each family calls them where its own checks stood, so
// which refusal comes first for several bad arguments is unchanged.
// ---------------------------------------------------------------------------------------------
inline bool check_create_common(const char* who, const void* cfg, const avexhip_tensor* tensors, int n_tensors) {
    if (!cfg || !tensors || n_tensors <= 0) { avexhip_set_error("%s: null config or empty weight table", who); return false; }
    if (avexhip_device_count() <= 0) { avexhip_set_error("%s: no HIP device visible (this path has no CPU fallback)", who); return false; }
    return true;
}
inline bool check_operand_dtype(const char* who, int dtype) {
    if (dtype == AVEXHIP_F16 || dtype == AVEXHIP_BF16) return true;
    avexhip_set_error("%s: unknown operand dtype %d", who, dtype);
    return false;
}
inline bool check_head64(const char* who, int E, int H) {      // avx::attention is built for 64-wide heads
    if (H > 0 && E == 64 * H) return true;
    avexhip_set_error("%s: head_dim must be 64 (E=%d, H=%d)", who, E, H);
    return false;
}
inline bool check_tile_dims(const char* who, int E, int F) {
    if (E % 128 == 0 && F % 128 == 0) return true;
    avexhip_set_error("%s: dims must be MFMA-tile multiples (E=%d F=%d)", who, E, F);
    return false;
}
// hook_mask / hook_out of a forward with hooks 0 .. n_hooks - 1; `noun` names what the bits count ("layer", "block", "tap"), `item` what
// a selected one is called ("hook"; EfficientNet: "tap")
inline int check_hooks(const char* who, const char* noun, uint32_t mask, float* const* out, int n_hooks, const char* item = "hook") {
    AVX_REQUIRE(mask == 0 || out, "%s: hook_mask set but hook_out is NULL", who);
    AVX_REQUIRE(n_hooks >= 32 || (mask >> n_hooks) == 0, "%s: hook_mask has bits beyond %s %d", who, noun, n_hooks - 1);
    for (int i = 0; i < n_hooks; ++i) AVX_REQUIRE(!((mask >> i) & 1u) || out[i], "%s: %s %d selected but hook_out[%d] is NULL", who, item, i, i);
    return AVEXHIP_OK;
}
inline int check_workspace(const char* who, const void* workspace, size_t given, size_t need) {
    if (workspace && given >= need) return AVEXHIP_OK;
    avexhip_set_error("%s: workspace too small (%zu bytes given, %zu needed)", who, given, need);
    return AVEXHIP_ERR_WORKSPACE;
}

// ---------------------------------------------------------------------------------------------
// The kaldi filterbank's window and mel bank as the reference builds them (beats.py:75,82-118), fp32 arithmetic
// ---------------------------------------------------------------------------------------------
inline void hann_window(int win, std::vector<float>& w) {      // torch.hann_window(win, periodic=False), the kaldi "hanning" window
    w.resize(win);
    for (int n = 0; n < win; ++n) w[n] = 0.5f - 0.5f * cosf((float)n * (float)(M_PI * 2.0 / (double)(win - 1)));
}
inline void kaldi_mel(int n_fft, int n_mels, float sr, float low, float high, std::vector<float>& fb) {
    const int nb = n_fft / 2;
    const float bin_w = sr / (float)n_fft;
    const float mel_low = (float)(1127.0 * log(1.0 + (double)low / 700.0));
    const float mel_high = (float)(1127.0 * log(1.0 + (double)high / 700.0));
    const float delta = (float)(((double)mel_high - (double)mel_low) / (double)(n_mels + 1));
    fb.assign((size_t)(nb + 1) * n_mels, 0.f);
    for (int m = 0; m < n_mels; ++m) {
        const float left = mel_low + (float)m * delta;
        const float center = mel_low + ((float)m + 1.0f) * delta;
        const float right = mel_low + ((float)m + 2.0f) * delta;
        for (int k = 0; k < nb; ++k) {
            const float f = bin_w * (float)k;
            const float mel = 1127.0f * logf(1.0f + f / 700.0f);
            const float up = (mel - left) / (center - left);
            const float down = (right - mel) / (right - center);
            fb[(size_t)k * n_mels + m] = fmaxf(0.f, fminf(up, down));
        }
    }
}

// name -> fp32 tensor table handed to *_create; a key matches with or without the wrapper prefixes of the reference's state dicts
struct Table {
    const avexhip_tensor* t;
    int n;
    const char* strip1 = "backbone.";      // avex/models/beats_model.py, eat_hf.py: self.backbone
    const char* strip2 = nullptr;          // e.g. "model." (EAT: backbone.model.*, AVES: model.*)
    const avexhip_tensor* find(const std::string& name) const {
        for (int i = 0; i < n; ++i) {
            if (!t[i].name) continue;
            const char* nm = t[i].name;
            if (strip1 && strncmp(nm, strip1, strlen(strip1)) == 0) nm += strlen(strip1);
            if (strip2 && strncmp(nm, strip2, strlen(strip2)) == 0) nm += strlen(strip2);
            if (name == nm) return &t[i];
        }
        return nullptr;
    }
};

// copy an fp32 tensor to the device (source may be host or device memory)
inline int dev_f32(HandleBase* h, const Table& tb, const std::string& name, int64_t numel, float** out, bool required = true) {
    const avexhip_tensor* t = tb.find(name);
    if (!t) {
        if (!required) { *out = nullptr; return AVEXHIP_OK; }
        avexhip_set_error("%s: tensor '%s' missing from the weight table", h->who, name.c_str());
        return AVEXHIP_ERR_MISSING;
    }
    if (t->numel != numel || !t->data) {
        avexhip_set_error("%s: tensor '%s' has %lld elements, expected %lld", h->who, name.c_str(), (long long)t->numel, (long long)numel);
        return AVEXHIP_ERR_INVALID;
    }
    float* d = nullptr;
    AVX_HIP_CHECK(hipMalloc((void**)&d, sizeof(float) * (size_t)numel));
    h->allocs.push_back(d);
    AVX_HIP_CHECK(hipMemcpy(d, t->data, sizeof(float) * (size_t)numel, hipMemcpyDefault));
    *out = d;
    return AVEXHIP_OK;
}

// gather an fp32 tensor of the table into a host vector (appending)
inline int host_f32(HandleBase* h, const Table& tb, const std::string& name, int64_t numel, std::vector<float>& out) {
    const avexhip_tensor* t = tb.find(name);
    if (!t || t->numel != numel || !t->data) {
        avexhip_set_error("%s: tensor '%s' missing or mis-sized", h->who, name.c_str());
        return AVEXHIP_ERR_MISSING;
    }
    const size_t o = out.size();
    out.resize(o + (size_t)numel);
    AVX_HIP_CHECK(hipMemcpy(out.data() + o, t->data, sizeof(float) * (size_t)numel, hipMemcpyDefault));
    return AVEXHIP_OK;
}

// host fp32 values -> half at dst (device), via a temporary fp32 device staging buffer
inline int upload_half(HandleBase* h, const float* host_or_dev, int64_t numel, void* dst, const char* what) {
    float* tmp = nullptr;
    AVX_HIP_CHECK(hipMalloc((void**)&tmp, sizeof(float) * (size_t)numel));
    hipError_t e = hipMemcpy(tmp, host_or_dev, sizeof(float) * (size_t)numel, hipMemcpyDefault);
    int rc = AVEXHIP_OK;
    if (e != hipSuccess) {
        avexhip_set_error("%s: copy of '%s' failed: %s", h->who, what, hipGetErrorString(e));
        rc = AVEXHIP_ERR_HIP;
    } else {
        rc = avx::cast_to_half(tmp, dst, numel, h->dtype, nullptr, h->d_ovf);      // (weights_fit below reads the counter when the handle is complete)
        if (rc == AVEXHIP_OK && hipDeviceSynchronize() != hipSuccess) {
            avexhip_set_error("%s: cast of '%s' failed", h->who, what);
            rc = AVEXHIP_ERR_HIP;
        }
    }
    (void)hipFree(tmp);
    return rc;
}

// fp32 tensor of the table -> half copy at dst (device)
inline int dev_half_into(HandleBase* h, const Table& tb, const std::string& name, int64_t numel, void* dst) {
    const avexhip_tensor* t = tb.find(name);
    if (!t) {
        avexhip_set_error("%s: tensor '%s' missing from the weight table", h->who, name.c_str());
        return AVEXHIP_ERR_MISSING;
    }
    if (t->numel != numel || !t->data) {
        avexhip_set_error("%s: tensor '%s' has %lld elements, expected %lld", h->who, name.c_str(), (long long)t->numel, (long long)numel);
        return AVEXHIP_ERR_INVALID;
    }
    return upload_half(h, (const float*)t->data, numel, dst, name.c_str());
}

inline int dev_half(HandleBase* h, const Table& tb, const std::string& name, int64_t numel, void** out) {
    void* d = nullptr;
    AVX_HIP_CHECK(hipMalloc(&d, 2 * (size_t)numel));
    h->allocs.push_back(d);
    *out = d;
    return dev_half_into(h, tb, name, numel, d);
}

// the weight-normed grouped positional convolution (K taps, G groups over E channels): fold g / v into one weight, packed for avx::posconv
inline int pack_posconv(HandleBase* h, const Table& tb, const std::string& name_g, const std::string& name_v, const std::string& name_bias, int E, int G,
                        int K, void** w_out, float** b_out) {
    const int cg = E / G;
    float *g = nullptr, *v = nullptr;
    AVXH_TRY(dev_f32(h, tb, name_g, K, &g));
    AVXH_TRY(dev_f32(h, tb, name_v, (int64_t)E * cg * K, &v));
    AVX_HIP_CHECK(hipMalloc(w_out, 2 * (size_t)E * cg * K));
    h->allocs.push_back(*w_out);
    AVXH_TRY(avx::posconv_pack(g, v, E, G, K, *w_out, h->dtype, nullptr));
    return dev_f32(h, tb, name_bias, E, b_out);
}

// W' = half(W * diag(gamma)), b' = b + W beta, s[n] = sum_k float(W'[n][k]) for a consumer of LayerNorm(y; gamma, beta)
// (W: [N, K] fp32 host rows gathered from the table by the caller)
inline int fold_ln(HandleBase* h, const std::vector<float>& W, const std::vector<float>& b, int N, int K, const float* gamma_dev,
                   const float* beta_dev, void** w_out, float** b_out, float** s_out) {
    std::vector<float> gamma(K), beta(K), Wg((size_t)N * K), bf(N);
    AVX_HIP_CHECK(hipMemcpy(gamma.data(), gamma_dev, sizeof(float) * K, hipMemcpyDefault));
    AVX_HIP_CHECK(hipMemcpy(beta.data(), beta_dev, sizeof(float) * K, hipMemcpyDefault));
    for (int n = 0; n < N; ++n) {
        double acc = b[n];
        const float* wr = &W[(size_t)n * K];
        float* wo = &Wg[(size_t)n * K];
        for (int k = 0; k < K; ++k) { wo[k] = wr[k] * gamma[k]; acc += (double)wr[k] * (double)beta[k]; }
        bf[n] = (float)acc;
    }
    float* tmp = nullptr;
    AVX_HIP_CHECK(hipMalloc((void**)&tmp, sizeof(float) * (size_t)N * K));
    void* wd = nullptr; float* bd = nullptr; float* sd = nullptr;
    int rc = AVEXHIP_OK;
    if (hipMalloc(&wd, 2 * (size_t)N * K) != hipSuccess || hipMalloc((void**)&bd, sizeof(float) * N) != hipSuccess ||
        hipMalloc((void**)&sd, sizeof(float) * N) != hipSuccess) {
        avexhip_set_error("%s: device allocation for folded weights failed", h->who);
        rc = AVEXHIP_ERR_HIP;
    }
    if (wd) h->allocs.push_back(wd);
    if (bd) h->allocs.push_back(bd);
    if (sd) h->allocs.push_back(sd);
    if (rc == AVEXHIP_OK && (hipMemcpy(tmp, Wg.data(), sizeof(float) * (size_t)N * K, hipMemcpyHostToDevice) != hipSuccess ||
                             hipMemcpy(bd, bf.data(), sizeof(float) * N, hipMemcpyHostToDevice) != hipSuccess)) {
        avexhip_set_error("%s: upload of folded weights failed", h->who);
        rc = AVEXHIP_ERR_HIP;
    }
    if (rc == AVEXHIP_OK) rc = avx::cast_to_half(tmp, wd, (int64_t)N * K, h->dtype, nullptr, h->d_ovf);
    if (rc == AVEXHIP_OK) rc = avx::row_sum_half(wd, N, K, sd, h->dtype, nullptr);
    if (rc == AVEXHIP_OK && hipDeviceSynchronize() != hipSuccess) { avexhip_set_error("%s: folding failed", h->who); rc = AVEXHIP_ERR_HIP; }
    (void)hipFree(tmp);
    *w_out = wd; *b_out = bd; *s_out = sd;
    return rc;
}

// ---------------------------------------------------------------------------------------------
// One post-LN transformer layer's parameters on the device
// ---------------------------------------------------------------------------------------------
struct Layer {
    void* w_qkv = nullptr; float* b_qkv = nullptr;
    void* w_o = nullptr;   float* b_o = nullptr;
    float* grep_w = nullptr; float* grep_b = nullptr; float* grep_a = nullptr;
    float* ln1_w = nullptr; float* ln1_b = nullptr;
    void* w_fc1 = nullptr; float* b_fc1 = nullptr;
    void* w_fc2 = nullptr; float* b_fc2 = nullptr;
    float* ln2_w = nullptr; float* ln2_b = nullptr;
    // LayerNorm-folded copies (see GemmArgs): fc1 consumes LN1 of this layer, QKV consumes LN2 of the previous layer
    void* w_fc1_f = nullptr; float* b_fc1_f = nullptr; float* s_fc1 = nullptr;
    void* w_qkv_f = nullptr; float* b_qkv_f = nullptr; float* s_qkv = nullptr;
    // residual-side folds (GemmArgs::lnr_prefolded): fc2 adds alpha * LN1(y1) of this layer, out_proj alpha * LN2(y2) of the previous layer;
    // ga = alpha * gamma, bb = bias + alpha * beta
    float* ga_fc2 = nullptr; float* bb_fc2 = nullptr;
    float* ga_o = nullptr; float* bb_o = nullptr;
};

// parameter names of layer i under a family's naming scheme ("%d" = layer index)
struct LayerNames {
    const char* qkv_fused;        // "blocks.%d.attn.qkv" ([3E, E] in one tensor), or NULL when q / k / v are separate:
    const char* q; const char* k; const char* v;
    const char* out_proj; const char* ln1; const char* fc1; const char* fc2; const char* ln2;
    const char* grep_linear; const char* grep_a;      // BEATs' gated relative position bias, or NULL
};

inline std::string fmt_name(const char* pattern, int i, const char* suffix) {
    char buf[256];
    snprintf(buf, sizeof(buf), pattern, i);
    return std::string(buf) + suffix;
}

struct CoreCfg {
    int E = 0, F = 0, H = 0, L = 0;   // F = 0: attention-only blocks, x = LN1(x + attn(x)) (the attention probe's layers, attention_probe.py:127-130)
    int head_dim = 64;                // 64: attention.hip (relative bias, gate, streaming); 32 / 96 / 128: attention_hd.hip (plain softmax attention)
    float alpha = 1.f, eps = 1e-5f;
    int hook_site = 0;            // 0: fc2's raw output, 1: the attention output projection's raw output
    bool fast = false;            // residual stream / pre-LN sums in the operand type
    bool fold = false;            // fast mode: the LayerNorms between the GEMMs folded into their epilogues (post-LN, GELU / SiLU FFN only)
    int fold_min_rows = 0;        // ... for chunks of at least this many token rows (default 4096; AVEX_AMD_LN_FOLD=1: 0 = always, so that a
                                  // clip's result never depends on the batch it came in)
    int act = 1;                  // GemmArgs::gelu code of the FFN activation (0 none, 1 erf GELU, 2 SiLU, 3 ReLU, 4 tanh GELU, 5 tanh)
    bool glu = false;             // fc1 is the reference's GLU_Linear(E, F, "swish"): one Linear to 2F, then value * swish(gate) (backbone.py:296-297)
    int hidden_shift = 0;         // > 0: fc1's hidden activations are stored x 2^-shift and fc2's weights packed x 2^shift (exact in the fp32 accumulation):
                                  // the f16 range ladder's rung for hidden activations beyond 65504 (the reference is fp32, backbone.py:365-370)
    bool pre_ln = false;          // pre-LN blocks (backbone.py:328-348): x += attn(LN1 x); x += ffn(LN2 x); `final_ln` after the stack (:146-147)
    bool batch_invariant = false; // residual_dtype bit 1 (AVEXHIP_RESIDUAL_BATCH_INVARIANT): a clip's outputs must not depend on the batch it arrives in --
                                  // fold at every size, no split-K, no LayerNorm inside a split-K epilogue, one final LayerNorm + pool path
    const float* final_ln_w = nullptr; const float* final_ln_b = nullptr;
};

// AVEX_AMD_LN_FOLD, read when a handle is created.  Unset / "auto": the encoder's LayerNorms are folded into the GEMMs around them (dims
// permitting) for chunks of >= 4096 token rows; smaller chunks run LayerNorm kernels.  Below that size the fold's 256-tile streaming kernel
// has a handful of tiles for 256 CUs and the 128-tile kernel (split-K for fc2) is quicker: one 10 s clip 2.17 -> 1.40 ms, four clips
// 2.22 -> 1.66, eight 2.28 -> 2.00; from sixteen clips on (7 936 rows) the fold is level or ahead (profiles/r03r_midsize.txt).
// "1": fold whatever the size -- a clip's embedding is then bit-identical whether it came alone or in a batch of 256 (with "auto" the two
// differ in their last bits, both inside the parity bar).  "0": never fold.
// residual_dtype of the handle configs: bit 0 = residual stream in the operand type, bit 1 = batch-invariant results
inline bool cfg_fast(int residual_dtype) { return (residual_dtype & 1) != 0; }
inline bool cfg_batch_invariant(int residual_dtype) {
    const char* e = getenv("AVEX_AMD_BATCH_INVARIANT");      // the environment can only turn it ON (for callers that cannot reach the config)
    return (residual_dtype & 2) != 0 || (e && atoi(e) != 0);
}
inline void fold_policy(bool fast, int E, int F, bool* fold, int* min_rows, bool batch_invariant = false) {
    const char* e = getenv("AVEX_AMD_LN_FOLD");
    const bool is_auto = !e || e[0] == 'a' || e[0] == 'A';
    *fold = fast && E % 256 == 0 && F % 256 == 0 && !(e && !is_auto && atoi(e) == 0);
    int rows = 4096;
    if (e && is_auto) { const char* c = strchr(e, ':'); if (c && atoi(c + 1) > 0) rows = atoi(c + 1); }      // "auto:4096": another threshold (experiments)
    *min_rows = is_auto && !batch_invariant ? rows : 0;
}
// a config's residual_dtype -> the CoreCfg fields it decides (reads AVEX_AMD_BATCH_INVARIANT, then AVEX_AMD_LN_FOLD: once, at create time)
inline void core_from_residual(CoreCfg& c, int residual_dtype, int E, int F) {
    c.fast = cfg_fast(residual_dtype);
    c.batch_invariant = cfg_batch_invariant(residual_dtype);
    fold_policy(c.fast, E, F, &c.fold, &c.fold_min_rows, c.batch_invariant);
}

// upload layer i (and, with the fold, its LayerNorm-folded copies; layer i - 1 must have been built)
inline int build_layer(HandleBase* h, const Table& tb, const LayerNames& nm, const CoreCfg& c, std::vector<Layer>& layers, int i) {
    const int E = c.E, F = c.F, H = c.H;
    Layer& ly = layers[i];
    AVX_HIP_CHECK(hipMalloc(&ly.w_qkv, 2 * (size_t)3 * E * E));
    h->allocs.push_back(ly.w_qkv);
    AVX_HIP_CHECK(hipMalloc((void**)&ly.b_qkv, sizeof(float) * 3 * E));
    h->allocs.push_back(ly.b_qkv);
    std::vector<float> Wqkv, bqkv;          // host copies: rows [0, E) are W_q (scaled by log2(e) here, in fp32), kept for the LayerNorm fold
    if (nm.qkv_fused) {
        AVXH_TRY(host_f32(h, tb, fmt_name(nm.qkv_fused, i, ".weight"), (int64_t)3 * E * E, Wqkv));
        AVXH_TRY(host_f32(h, tb, fmt_name(nm.qkv_fused, i, ".bias"), 3 * E, bqkv));
    } else {
        const char* part[3] = {nm.q, nm.k, nm.v};
        for (int j = 0; j < 3; ++j) {
            AVXH_TRY(host_f32(h, tb, fmt_name(part[j], i, ".weight"), (int64_t)E * E, Wqkv));
            AVXH_TRY(host_f32(h, tb, fmt_name(part[j], i, ".bias"), E, bqkv));
        }
    }
    if (h->q_log2e) {
        const float l2e = 1.4426950408889634f;
        for (size_t j = 0; j < (size_t)E * E; ++j) Wqkv[j] *= l2e;
        for (int j = 0; j < E; ++j) bqkv[j] *= l2e;
    }
    AVXH_TRY(upload_half(h, Wqkv.data(), (int64_t)3 * E * E, ly.w_qkv, "qkv.weight"));
    AVX_HIP_CHECK(hipMemcpy(ly.b_qkv, bqkv.data(), sizeof(float) * 3 * E, hipMemcpyHostToDevice));
    AVXH_TRY(dev_half(h, tb, fmt_name(nm.out_proj, i, ".weight"), (int64_t)E * E, &ly.w_o));
    AVXH_TRY(dev_f32(h, tb, fmt_name(nm.out_proj, i, ".bias"), E, &ly.b_o));
    if (nm.grep_linear) {
        AVXH_TRY(dev_f32(h, tb, fmt_name(nm.grep_linear, i, ".weight"), 8 * (E / H), &ly.grep_w));
        AVXH_TRY(dev_f32(h, tb, fmt_name(nm.grep_linear, i, ".bias"), 8, &ly.grep_b));
        AVXH_TRY(dev_f32(h, tb, fmt_name(nm.grep_a, i, ""), H, &ly.grep_a));
    }
    AVXH_TRY(dev_f32(h, tb, fmt_name(nm.ln1, i, ".weight"), E, &ly.ln1_w));
    AVXH_TRY(dev_f32(h, tb, fmt_name(nm.ln1, i, ".bias"), E, &ly.ln1_b));
    if (F == 0) return AVEXHIP_OK;         // attention-only block
    const int F1 = c.glu ? 2 * F : F;      // GLU_Linear keeps its Linear(E, 2F) under ".linear"
    AVXH_TRY(dev_half(h, tb, fmt_name(nm.fc1, i, c.glu ? ".linear.weight" : ".weight"), (int64_t)F1 * E, &ly.w_fc1));
    AVXH_TRY(dev_f32(h, tb, fmt_name(nm.fc1, i, c.glu ? ".linear.bias" : ".bias"), F1, &ly.b_fc1));
    if (c.hidden_shift > 0) {
        // fc2's weights x 2^shift: the power of two is exact in fp32 and in the operand type unless a weight leaves its range
        std::vector<float> W2;
        AVXH_TRY(host_f32(h, tb, fmt_name(nm.fc2, i, ".weight"), (int64_t)E * F, W2));
        const float sc = ldexpf(1.0f, c.hidden_shift);
        float mx = 0.f;
        for (float& v : W2) { v *= sc; mx = fabsf(v) > mx ? fabsf(v) : mx; }
        if (h->dtype == AVEXHIP_F16 && !(mx <= 65504.0f)) {
            avexhip_set_error("%s: hidden_shift %d takes layer %d's fc2 weights out of the f16 range (max |w| 2^shift = %g)", h->who, c.hidden_shift, i, (double)mx);
            return AVEXHIP_ERR_INVALID;
        }
        AVX_HIP_CHECK(hipMalloc(&ly.w_fc2, 2 * (size_t)E * F));
        h->allocs.push_back(ly.w_fc2);
        AVXH_TRY(upload_half(h, W2.data(), (int64_t)E * F, ly.w_fc2, "fc2.weight x 2^shift"));
    } else {
        AVXH_TRY(dev_half(h, tb, fmt_name(nm.fc2, i, ".weight"), (int64_t)E * F, &ly.w_fc2));
    }
    AVXH_TRY(dev_f32(h, tb, fmt_name(nm.fc2, i, ".bias"), E, &ly.b_fc2));
    AVXH_TRY(dev_f32(h, tb, fmt_name(nm.ln2, i, ".weight"), E, &ly.ln2_w));
    AVXH_TRY(dev_f32(h, tb, fmt_name(nm.ln2, i, ".bias"), E, &ly.ln2_b));
    if (c.fold) {
        auto two = [&](float** ga, float** bb) -> int {
            AVX_HIP_CHECK(hipMalloc((void**)ga, sizeof(float) * 2 * (size_t)E));
            h->allocs.push_back(*ga);
            *bb = *ga + E;
            return AVEXHIP_OK;
        };
        AVXH_TRY(two(&ly.ga_fc2, &ly.bb_fc2));
        AVXH_TRY(avx::lnr_fold(ly.ln1_w, ly.ln1_b, ly.b_fc2, c.alpha, E, ly.ga_fc2, ly.bb_fc2, nullptr));
        std::vector<float> Wh, bh;
        AVXH_TRY(host_f32(h, tb, fmt_name(nm.fc1, i, ".weight"), (int64_t)F * E, Wh));
        AVXH_TRY(host_f32(h, tb, fmt_name(nm.fc1, i, ".bias"), F, bh));
        AVXH_TRY(fold_ln(h, Wh, bh, F, E, ly.ln1_w, ly.ln1_b, &ly.w_fc1_f, &ly.b_fc1_f, &ly.s_fc1));
        if (i > 0) {   // QKV and out_proj of layer i read LN2 of layer i - 1
            const Layer& prev = layers[i - 1];
            AVXH_TRY(two(&ly.ga_o, &ly.bb_o));
            AVXH_TRY(avx::lnr_fold(prev.ln2_w, prev.ln2_b, ly.b_o, c.alpha, E, ly.ga_o, ly.bb_o, nullptr));
            AVXH_TRY(fold_ln(h, Wqkv, bqkv, 3 * E, E, prev.ln2_w, prev.ln2_b, &ly.w_qkv_f, &ly.b_qkv_f, &ly.s_qkv));
        }
    }
    return AVEXHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// The layer loop's buffers inside a caller-provided workspace, and the loop itself
// ---------------------------------------------------------------------------------------------
struct CoreWs {
    float* x; char* xh; float* pre; char* preh; char* qkv; char* ah; char* hh; float* raw;
    char* hh2;                // GLU: fc1's [M, 2F] output before the gate
    float* pool;              // mean-pooled hook taps: per-block column sums [ceil(M / 64)][2][E] (GemmArgs::pool_part)
    float* splitk; size_t splitk_bytes;      // split-K partials of the few-row products (GemmArgs::splitk_ws): 8 x min(M, 1024) x E floats
    float* st1; float* st2;   // folded LayerNorm: per-row partial statistics [M][E/64][2] of y1 (preh) and y2 (xh)
    float* r1; float* r2;     // ... reduced to (rstd, -mu rstd) per row by avx::ln_rowstats
};

inline CoreWs carve_core(const CoreCfg& c, size_t M, Carver& cv) {
    CoreWs w;
    w.x = (float*)cv.take(M * c.E * 4);
    w.xh = (char*)cv.take(M * c.E * 2);
    w.pre = (float*)cv.take(c.fast ? 256 : M * c.E * 4);
    w.preh = (char*)cv.take(c.fast ? M * c.E * 2 : 256);
    w.qkv = (char*)cv.take(M * 3 * c.E * 2);
    w.ah = (char*)cv.take(M * c.E * 2);
    w.hh = (char*)cv.take(M * c.F * 2);
    w.hh2 = (char*)cv.take(c.glu ? M * c.F * 4 : 256);
    w.pool = (float*)cv.take(((M + 63) / 64) * 2 * (size_t)c.E * 4);
    w.splitk_bytes = (8 * M < 16384 ? 8 * M : 16384) * (size_t)c.E * 4;      // 8 splits up to 2 048 rows, 2 up to 8 192
    w.splitk = (float*)cv.take(w.splitk_bytes);
    w.raw = (float*)cv.take(M * c.E * 4);
    w.st1 = (float*)cv.take(c.fold ? M * (c.E / 64) * 8 : 256);
    w.st2 = (float*)cv.take(c.fold ? M * (c.E / 64) * 8 : 256);
    w.r1 = (float*)cv.take(c.fold ? (M + 256) * 8 : 256);
    w.r2 = (float*)cv.take(c.fold ? (M + 256) * 8 : 256);
    return w;
}

struct CoreIo {
    int Bc = 0, Tt = 0;
    size_t c0 = 0;                        // first clip of this chunk within the caller's batch (offset of the outputs)
    const float* bias_tab = nullptr;      // [H, 2 Tt - 1] or NULL
    const uint8_t* pad = nullptr;         // [Bc, Tt] key padding or NULL
    uint32_t hook_mask = 0;               // bit (hook_bit0 + i) selects layer i
    int hook_bit0 = 0;
    float* const* hook_out = nullptr;     // indexed like the mask's bits
    int hook_pooled = 0;
    float* features_out = nullptr;        // caller's [B, Tt, E] or NULL
    float* pooled_out = nullptr;          // caller's [B, E] (mean over the Tt tokens) or NULL
    float* final_f32 = nullptr;           // out: where the fp32 features of this chunk were written (caller's buffer or w.x), NULL if nowhere
};

// A hooked GEMM: the raw tap goes to the caller's [B, T, E] buffer, or -- mean-pooled taps of clips with >= 64 tokens on the 256-tile
// kernel -- never exists: the epilogue leaves per-block column sums and tap_finish reduces them to [B, E].  Shorter clips / narrow
// outputs write the tap to scratch and pool it from there.
struct Tap {
    bool hooked = false, fused = false;
    float* out = nullptr;      // caller's buffer for this chunk
};
inline Tap tap_begin(const CoreCfg& c, const CoreWs& w, const CoreIo& io, int layer, avx::GemmArgs& g) {
    Tap t;
    t.hooked = (io.hook_mask >> (io.hook_bit0 + layer)) & 1u;
    if (!t.hooked) return t;
    const size_t per_clip = io.hook_pooled ? (size_t)c.E : (size_t)io.Tt * c.E;
    t.out = io.hook_out[io.hook_bit0 + layer] + io.c0 * per_clip;
    static const bool no_fuse = getenv("AVEX_AMD_POOL_FUSE") && atoi(getenv("AVEX_AMD_POOL_FUSE")) == 0;
    // io.hook_pooled: 1 mean, 2 max, 3 first token over a clip's rows (extract_embeddings' aggregations, beats_model.py:403-417)
    // ... where that kernel is the one the product takes anyway (a folded LayerNorm, or enough tiles): a pooled tap must not change which
    // kernel computes the layer, or its max / first-token values would differ in their last bits from the same reduction of the full tap
    const bool streams = g.ln_rows || g.lnr_y || g.stats_out || avx::gemm_streams(g.M, g.N);
    // batch-invariant handles do not fuse the MEAN: its partial sums are grouped by 64-row blocks of the whole batch, so a clip's mean would
    // depend on where the clip starts (maxima and first rows are exact and stay fused)
    t.fused = io.hook_pooled && io.Tt >= 64 && c.E % 256 == 0 && g.K >= 128 && streams && !no_fuse && !(c.batch_invariant && io.hook_pooled == 1);
    if (t.fused) {
        g.pool_T = io.Tt; g.pool_mode = io.hook_pooled - 1;
        g.pool_part = io.hook_pooled == 3 ? t.out : w.pool;      // the first rows go straight to the caller's [B, E]
    } else { g.out_raw = io.hook_pooled ? w.raw : t.out; g.ldraw = c.E; }
    return t;
}
inline int tap_finish(const Tap& t, const CoreCfg& c, const CoreWs& w, const CoreIo& io, hipStream_t cs) {
    if (!t.hooked || !io.hook_pooled) return AVEXHIP_OK;
    if (t.fused) return io.hook_pooled == 3 ? AVEXHIP_OK : avx::pool_reduce(w.pool, io.Bc, io.Tt, c.E, t.out, c.E, cs, io.hook_pooled - 1);
    return avx::agg_pool(w.raw, io.Bc, io.Tt, c.E, io.hook_pooled, t.out, cs);
}

// batch-invariant handles: every layer product in the 256-tile streaming kernel whatever its row count (the 128-tile kernel's residual
// epilogue multiplies and adds where the streaming kernel's fuses, and its split-K adds in another order)
inline void pin_kernel(const CoreCfg& c, avx::GemmArgs& g) {
    if (c.batch_invariant && g.variant == 0 && g.M >= 2 && avx::gemm_streaming_takes(g)) g.variant = 5;
}

inline int self_attention(HandleBase* h, const CoreCfg& c, const Layer& ly, const CoreWs& w, const CoreIo& io, hipStream_t cs) {
    if (c.head_dim == 64)
        return avx::attention(w.qkv, io.Bc, io.Tt, c.H, io.bias_tab, ly.grep_w, ly.grep_b, ly.grep_a, io.pad, w.ah, h->dtype, cs, h->q_log2e ? 1 : 0);
    return avx::attention_hd(w.qkv, io.Bc, io.Tt, c.H, c.head_dim, io.pad, w.ah, h->dtype, cs, h->q_log2e ? 1 : 0);
}

// fc1 (+ activation) of a prepared GemmArgs `g` (A, W, bias, fold fields set; N = F, output w.hh): plain, or the gated linear unit
inline int ffn_hidden(HandleBase* h, const CoreCfg& c, const CoreWs& w, avx::GemmArgs& g, int M, Prof& prof, hipStream_t cs) {
    const double flops = 2.0 * (double)M * (c.glu ? 2 * c.F : c.F) * c.E;
    int rc;
    if (c.glu) { g.N = 2 * c.F; g.gelu = 0; g.out_half = w.hh2; g.ldh = 2 * c.F; }
    if (c.hidden_shift > 0) g.half_scale = ldexpf(1.0f, -c.hidden_shift);      // (refused with GLU when the handle is created)
    prof.begin("gemm.fc1", flops);
    pin_kernel(c, g);
    rc = avx::gemm(g, h->dtype, cs);
    prof.end();
    if (rc != AVEXHIP_OK || !c.glu) return rc;
    prof.begin("glu", 0.0);
    rc = avx::glu_swish(w.hh2, M, c.F, w.hh, h->d_ovf, h->dtype, cs);
    prof.end();
    return rc;
}

// The residual stream where a product reads or writes it: fp32, or the operand type (fast handles) -- one of the two pointers
struct Stream { float* f32; void* half; };
// what the LayerNorm fold (run_layers) changes in a layer's products
struct Fold {
    bool on = false;          // y1 / y2 stay raw with row statistics; fc1 and fc2 read LayerNorm 1 through them
    bool raw_in = false;      // ... and the layer's input is the previous layer's raw y2 (QKV and out_proj read LayerNorm 2 through it)
    bool last = false;        // the last layer's y2 goes to a LayerNorm kernel that takes its own statistics
};

// ---- the four products of a layer, each set up in one place ---------------------------------------------------------------------
// out = alpha * residual + product: the stream in and out; with `lnr_rows` (fold) src holds raw rows whose LayerNorm is the residual, applied on the fly
inline void residual_args(avx::GemmArgs& g, const CoreCfg& c, Stream src, Stream dst, const float* lnr_rows = nullptr, const float* ga = nullptr, const float* bb = nullptr) {
    g.alpha = c.alpha;
    if (dst.half) { g.out_half = dst.half; g.ldh = c.E; } else { g.out_f32 = dst.f32; g.ldo = c.E; }
    if (lnr_rows) { g.lnr_y = src.half; g.ldy = c.E; g.lnr_rows = lnr_rows; g.lnr_gamma = ga; g.lnr_beta = bb; g.lnr_prefolded = 1; }
    else if (src.half) { g.resid_half = src.half; g.ldrh = c.E; }
    else { g.resid = src.f32; g.ldr = c.E; }
}
inline void qkv_args(avx::GemmArgs& g, const HandleBase* h, const CoreCfg& c, const Layer& ly, const CoreWs& w, int M, const void* A, const Fold& f) {
    gemm_init(g, h);
    g.A = A; g.lda = c.E; g.W = ly.w_qkv; g.ldw = c.E; g.M = M; g.N = 3 * c.E; g.K = c.E; g.bias = ly.b_qkv;
    g.out_half = w.qkv; g.ldh = 3 * c.E;
    if (f.raw_in) { g.W = ly.w_qkv_f; g.bias = ly.b_qkv_f; g.ln_rows = w.r2; g.ln_s = ly.s_qkv; }
}
inline void out_proj_args(avx::GemmArgs& g, const HandleBase* h, const CoreCfg& c, const Layer& ly, const CoreWs& w, int M, Stream src, Stream dst, const Fold& f) {
    gemm_init(g, h);
    g.A = w.ah; g.lda = c.E; g.W = ly.w_o; g.ldw = c.E; g.M = M; g.N = c.E; g.K = c.E; g.bias = ly.b_o;
    if (f.raw_in) residual_args(g, c, src, dst, w.r2, ly.ga_o, ly.bb_o);
    else residual_args(g, c, src, dst);
    if (f.on) { g.stats_out = w.st1; g.rows_out = w.r1; g.rows_eps = c.eps; }      // LN1's row statistics with the product (avx::gemm runs ln_rowstats behind it)
}
inline void fc1_args(avx::GemmArgs& g, const HandleBase* h, const CoreCfg& c, const Layer& ly, const CoreWs& w, int M, const void* A, const Fold& f) {
    gemm_init(g, h);
    g.A = A; g.lda = c.E; g.W = ly.w_fc1; g.ldw = c.E; g.M = M; g.N = c.F; g.K = c.E; g.bias = ly.b_fc1; g.gelu = c.act;
    g.out_half = w.hh; g.ldh = c.F;
    if (f.on) { g.W = ly.w_fc1_f; g.bias = ly.b_fc1_f; g.ln_rows = w.r1; g.ln_s = ly.s_fc1; }
}
inline void fc2_args(avx::GemmArgs& g, const HandleBase* h, const CoreCfg& c, const Layer& ly, const CoreWs& w, int M, Stream src, Stream dst, const Fold& f) {
    gemm_init(g, h);
    g.A = w.hh; g.lda = c.F; g.W = ly.w_fc2; g.ldw = c.F; g.M = M; g.N = c.E; g.K = c.F; g.bias = ly.b_fc2;
    if (M <= 8192 && !c.batch_invariant) { g.splitk_ws = w.splitk; g.splitk_bytes = w.splitk_bytes; }      // (split-K adds in another order than one pass over K)
    if (f.on) {
        residual_args(g, c, src, dst, w.r1, ly.ga_fc2, ly.bb_fc2);
        g.stats_out = !f.last ? w.st2 : nullptr;
    } else residual_args(g, c, src, dst);
}
// LayerNorm in the split-K epilogue of the product (one kernel less; the caller asked avx::gemm_post_ln_ok)
inline void post_ln_args(avx::GemmArgs& g, const CoreCfg& c, const float* ln_w, const float* ln_b, float* out_f32, void* out_half) {
    g.post_ln_w = ln_w; g.post_ln_b = ln_b; g.post_ln_eps = c.eps; g.post_ln_round = c.fast ? 1 : 0;
    g.post_ln_out_f32 = out_f32; g.post_ln_ldo = c.E; g.post_ln_out_half = out_half; g.post_ln_ldh = c.E;
}
inline int layer_gemm(HandleBase* h, const CoreCfg& c, avx::GemmArgs& g, const char* stage, double flops, Prof& prof, hipStream_t cs) {
    prof.begin(stage, flops);
    pin_kernel(c, g);
    AVXH_TRY(avx::gemm(g, h->dtype, cs));
    prof.end();
    return AVEXHIP_OK;
}

// ---- the outputs of the stack: the final LayerNorm of the stream -> fp32 features and / or their mean over tokens -----------------
struct Tail {
    bool fused_pool = false;      // pooled embedding only (the headline path): LayerNorm and the mean over tokens in one pass, no fp32 feature tensor
    float* xo = nullptr;          // the fp32 features: the caller's buffer, scratch when something reads them, or nowhere
    bool ln_stage = false;        // a "layernorm" profile stage even where no LayerNorm kernel runs (the post-LN loop without the fold records one per layer)
};
inline Tail tail_begin(const CoreCfg& c, const CoreWs& w, const CoreIo& io, bool may_fuse_pool, bool scratch_anyway) {
    Tail t;
    t.fused_pool = may_fuse_pool && io.pooled_out && !io.features_out && c.fast && c.E % 8 == 0 && c.E <= 768 && (io.Bc >= 32 || c.batch_invariant);
    t.xo = io.features_out ? io.features_out + io.c0 * io.Tt * c.E : ((io.pooled_out || scratch_anyway) ? w.x : nullptr);
    return t;
}
// y: the un-normalised stream.  ln_done: the LayerNorm rode in the epilogue of the product that wrote y
inline int tail_finish(HandleBase* h, const CoreCfg& c, CoreIo& io, const Tail& t, Stream y, const float* ln_w, const float* ln_b, bool ln_done, Prof& prof, hipStream_t cs) {
    const int E = c.E, M = io.Bc * io.Tt;
    if (t.fused_pool) {
        prof.begin("layernorm+mean_pool", 0.0);
        AVXH_TRY(avx::layernorm_pool(y.half, E, ln_w, ln_b, c.eps, io.Bc, io.Tt, E, io.pooled_out + io.c0 * E, h->dtype, cs));
        prof.end();
        return AVEXHIP_OK;
    }
    if (t.xo || t.ln_stage) {
        prof.begin("layernorm", 0.0);
        if (t.xo && !ln_done) AVXH_TRY(avx::layernorm(y.f32, y.half, E, ln_w, ln_b, c.eps, M, E, t.xo, E, nullptr, E, h->dtype, cs));
        prof.end();
    }
    io.final_f32 = t.xo;
    if (io.pooled_out) {
        prof.begin("mean_pool", 0.0);
        AVXH_TRY(avx::mean_pool(t.xo, io.Bc, io.Tt, E, io.pooled_out + io.c0 * E, cs));
        prof.end();
    }
    return AVEXHIP_OK;
}

// Pre-LN blocks (backbone.py:328-348).  The un-normalised stream starts in w.pre (fp32 residual stream) / w.preh (fast) -- where the
// positional convolution left x + pos_conv(x) -- and is back there after every layer; each LayerNorm writes the GEMM operand to w.ah.
inline int run_layers_pre_ln(HandleBase* h, const CoreCfg& c, const std::vector<Layer>& layers, const CoreWs& w, CoreIo& io, Prof& prof, hipStream_t cs) {
    const int E = c.E, F = c.F, H = c.H, L = c.L, dt = h->dtype, Tt = io.Tt;
    const int M = io.Bc * Tt;
    const double Md = (double)M;
    const Stream s0 = c.fast ? Stream{nullptr, w.preh} : Stream{w.pre, nullptr};      // stream at layer boundaries
    const Stream s1 = c.fast ? Stream{nullptr, w.xh} : Stream{w.x, nullptr};          // stream after the attention block
    const Fold no_fold;
    avx::GemmArgs g;
    io.final_f32 = nullptr;
    for (int i = 0; i < L; ++i) {
        const Layer& ly = layers[i];
        prof.begin("layernorm", 0.0);
        AVXH_TRY(avx::layernorm(s0.f32, s0.half, E, ly.ln1_w, ly.ln1_b, c.eps, M, E, nullptr, E, w.ah, E, dt, cs));
        prof.end();
        qkv_args(g, h, c, ly, w, M, w.ah, no_fold);
        AVXH_TRY(layer_gemm(h, c, g, "gemm.qkv", 2.0 * Md * 3 * E * E, prof, cs));
        prof.begin("attention", 4.0 * Md * Tt * E + (ly.grep_w ? 2.0 * Md * 8 * (E / H) * H : 0.0));
        AVXH_TRY(self_attention(h, c, ly, w, io, cs));
        prof.end();
        out_proj_args(g, h, c, ly, w, M, s0, s1, no_fold);
        Tap tap_o;
        if (c.hook_site == 1) tap_o = tap_begin(c, w, io, i, g);
        AVXH_TRY(layer_gemm(h, c, g, "gemm.out_proj", 2.0 * Md * E * E, prof, cs));
        AVXH_TRY(tap_finish(tap_o, c, w, io, cs));
        prof.begin("layernorm", 0.0);
        AVXH_TRY(avx::layernorm(s1.f32, s1.half, E, ly.ln2_w, ly.ln2_b, c.eps, M, E, nullptr, E, w.ah, E, dt, cs));
        prof.end();
        fc1_args(g, h, c, ly, w, M, w.ah, no_fold);
        AVXH_TRY(ffn_hidden(h, c, w, g, M, prof, cs));
        fc2_args(g, h, c, ly, w, M, s1, s0, no_fold);
        Tap tap_f;
        if (c.hook_site == 0) tap_f = tap_begin(c, w, io, i, g);
        AVXH_TRY(layer_gemm(h, c, g, "gemm.fc2", 2.0 * Md * E * F, prof, cs));
        AVXH_TRY(tap_finish(tap_f, c, w, io, cs));
    }
    // the encoder's LayerNorm after the stack (backbone.py:146-147)
    if (L > 0 && (io.features_out || io.pooled_out)) AVXH_TRY(tail_finish(h, c, io, tail_begin(c, w, io, true, false), s0, c.final_ln_w, c.final_ln_b, false, prof, cs));
    return AVEXHIP_OK;
}

// x (the encoder input after its own LayerNorm) is in w.xh (fast) / w.x + w.xh (fp32 residual stream); runs the L layers and the outputs
inline int run_layers(HandleBase* h, const CoreCfg& c, const std::vector<Layer>& layers, const CoreWs& w, CoreIo& io, Prof& prof, hipStream_t cs) {
    const int E = c.E, F = c.F, H = c.H, L = c.L, dt = h->dtype, Tt = io.Tt;
    const int M = io.Bc * Tt;
    const double Md = (double)M;
    const bool fast = c.fast;
    if (c.pre_ln) return run_layers_pre_ln(h, c, layers, w, io, prof, cs);
    float* x32 = fast ? nullptr : w.x;      // the fp32 copy of x beside w.xh (fp32 residual stream only)
    const Stream x = fast ? Stream{nullptr, w.xh} : Stream{w.x, nullptr};          // the stream at layer boundaries and after LayerNorm 1
    const Stream pre = fast ? Stream{nullptr, w.preh} : Stream{w.pre, nullptr};    // the sums y1 / y2 before their LayerNorms
    // "fold": the two LayerNorms of a layer never run as kernels.  y1 = x*alpha + attn (preh) and y2 = x1*alpha + ffn (xh) stay raw
    // in the operand type with per-row partial statistics from the epilogue that wrote them; fc1 / the next QKV read them
    // through LayerNorm-folded weights, out_proj / fc2 apply LayerNorm to their residual on the fly (GemmArgs, gemm.hip).
    Fold f;
    f.on = fast && c.fold && F > 0 && M >= c.fold_min_rows;      // default: any M, the same arithmetic whatever the chunking
    const bool few_rows = !f.on && M <= 8192 && !c.batch_invariant;      // LayerNorms may ride in split-K epilogues
    avx::GemmArgs g;
    io.final_f32 = nullptr;
    for (int i = 0; i < L; ++i) {
        const Layer& ly = layers[i];
        const bool last = i == L - 1;
        f.raw_in = f.on && i > 0;      // xh holds y2 of layer i-1 (raw) instead of its LayerNorm
        f.last = last;
        qkv_args(g, h, c, ly, w, M, w.xh, f);
        AVXH_TRY(layer_gemm(h, c, g, "gemm.qkv", 2.0 * Md * 3 * E * E, prof, cs));
        prof.begin("attention", 4.0 * Md * Tt * E + (ly.grep_w ? 2.0 * Md * 8 * (E / H) * H : 0.0));
        AVXH_TRY(self_attention(h, c, ly, w, io, cs));
        prof.end();
        out_proj_args(g, h, c, ly, w, M, x, pre, f);
        Tap tap_o;
        if (c.hook_site == 1) tap_o = tap_begin(c, w, io, i, g);
        // few rows, no fold: LayerNorm 1 rides in the split-K epilogue of the product (one kernel less per layer; x32 / xh are read as the
        // residual and rewritten row by row by the same wave)
        bool ln1_fused = false;
        if (few_rows && F > 0) {
            g.splitk_ws = w.splitk; g.splitk_bytes = w.splitk_bytes;
            ln1_fused = avx::gemm_post_ln_ok(g);
            if (ln1_fused) post_ln_args(g, c, ly.ln1_w, ly.ln1_b, x32, w.xh);
            else { g.splitk_ws = nullptr; g.splitk_bytes = 0; }
        }
        AVXH_TRY(layer_gemm(h, c, g, "gemm.out_proj", 2.0 * Md * E * E, prof, cs));
        AVXH_TRY(tap_finish(tap_o, c, w, io, cs));
        if (F == 0) {      // attention-only block: LN1 closes it
            if (last) { AVXH_TRY(tail_finish(h, c, io, tail_begin(c, w, io, false, true), pre, ly.ln1_w, ly.ln1_b, false, prof, cs)); continue; }
            prof.begin("layernorm", 0.0);
            AVXH_TRY(avx::layernorm(pre.f32, pre.half, E, ly.ln1_w, ly.ln1_b, c.eps, M, E, x32, E, w.xh, E, dt, cs));
            prof.end();
            continue;
        }
        if (!f.on && !ln1_fused) {      // (fold: w.r1 = LN1's (rstd, -mu rstd) came out of the product: GemmArgs::rows_out)
            prof.begin("layernorm", 0.0);
            AVXH_TRY(avx::layernorm(pre.f32, pre.half, E, ly.ln1_w, ly.ln1_b, c.eps, M, E, x32, E, w.xh, E, dt, cs));
            prof.end();
        }
        fc1_args(g, h, c, ly, w, M, f.on ? w.preh : w.xh, f);
        AVXH_TRY(ffn_hidden(h, c, w, g, M, prof, cs));
        // fold: residual = LN1(y1) on the fly; y2 (raw) goes to xh, which nothing reads any more in this layer
        const Stream y2 = f.on ? x : pre;
        fc2_args(g, h, c, ly, w, M, f.on ? pre : x, y2, f);
        Tap tap_f;
        if (c.hook_site == 0) tap_f = tap_begin(c, w, io, i, g);
        // LayerNorm 2 makes the next layer's x -- or, after the last layer, the outputs
        Tail tail;
        if (last) tail = tail_begin(c, w, io, true, !fast);
        else tail.xo = x32;
        tail.ln_stage = !f.on;
        // few rows, no fold: LayerNorm 2 in the split-K epilogue (as LayerNorm 1 above)
        const bool ln2_fused = !f.on && !tail.fused_pool && (tail.xo || !last) && avx::gemm_post_ln_ok(g);
        if (ln2_fused) post_ln_args(g, c, ly.ln2_w, ly.ln2_b, tail.xo, last ? nullptr : w.xh);
        AVXH_TRY(layer_gemm(h, c, g, "gemm.fc2", 2.0 * Md * E * F, prof, cs));
        AVXH_TRY(tap_finish(tap_f, c, w, io, cs));
        if (last) { AVXH_TRY(tail_finish(h, c, io, tail, y2, ly.ln2_w, ly.ln2_b, ln2_fused, prof, cs)); continue; }
        if (f.on) {
            prof.begin("ln_rowstats", 0.0);
            AVXH_TRY(avx::ln_rowstats(w.st2, M, E / 64, c.eps, w.r2, cs));
            prof.end();
        } else {
            prof.begin("layernorm", 0.0);
            if (!ln2_fused) AVXH_TRY(avx::layernorm(pre.f32, pre.half, E, ly.ln2_w, ly.ln2_b, c.eps, M, E, x32, E, w.xh, E, dt, cs));
            prof.end();
        }
    }
    return AVEXHIP_OK;
}

}  // namespace avxh
